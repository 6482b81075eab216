/*
 * sdf_abi.h -- C-ABI of the MI355X-native SDF sphere-tracing renderer.
 *
 * This is the drop-in boundary that replaces the reference's device programs
 * (ezorzin/SDF3D `Code/shader/voxel_fragment.frag`, `voxel_geometry.geom`,
 * `voxel_vertex.vert` and the never-enqueued `Code/kernel/thekernel_1.cl`).
 * Plain C: POD structs, plain pointers and sizes, integer status codes.  No
 * torch / C++ types cross this boundary.
 *
 * Reference interface each entry point replaces (paths relative to the
 * reference root):
 *
 *   sdf_defaults()   the hard-coded constants and scene of the fragment shader:
 *                    voxel_fragment.frag:15-23 (PI, MAX_STEPS, MAX_DISTANCE,
 *                    EPSILON), :54-81 (sphere + plane, hard union), :178-189
 *                    (camera, light, material), :205 (shadow k = 10); and the
 *                    host's default window / view (main.cpp:4-11: 800x600,
 *                    orbit and pan at 0 -> V_mat = identity).
 *   sdf_render()     one frame of `gl->plot(sh, proj_mode)` (main.cpp:95), i.e.
 *                    the fragment stage `main()` (voxel_fragment.frag:160-211)
 *                    run once per pixel, with the pixel -> `quad` mapping of
 *                    voxel_geometry.geom:26-52 folded into the index math, and
 *                    with the uniforms `V_mat`, `AR` (voxel_fragment.frag:5-7)
 *                    passed explicitly in sdf_camera.  The output is the
 *                    shader's `fragment_color` (:12, :210) as float RGBA.
 *   sdf_deinterleave() gathers per-device row blocks into one frame (new: the
 *                    reference has a single GL context, main.cpp:48,53).
 *   sdf_driver_*()   the multi-device frame loop: the reference's per-frame
 *                    `gl->plot` loop (main.cpp:87-98) run across the GPUs of
 *                    one node, every rank rendering its row blocks and rank 0
 *                    assembling the frame over RCCL (new: the reference has a
 *                    single GL context, main.cpp:48,53).
 *   sdf_strerror()   error text (the reference has none: main.cpp:109).
 *
 * Conventions
 *   - Framebuffer: width x height pixels, 4 floats (R,G,B,A) per pixel,
 *     row-major, row 0 = BOTTOM row (GL window origin), pixel (x, y) at
 *     rgba[(y * width + x) * 4].
 *   - Matrices: 16 floats, column-major, exactly like a GLSL mat4 uniform.
 *   - All device pointers are HIP device pointers on the current device; the
 *     call is asynchronous on `stream` (a hipStream_t, NULL = null stream).
 *   - Functions return SDF_OK (0) or a negative SDF_E* code; they never throw.
 */
#ifndef SDF_ABI_H
#define SDF_ABI_H

#ifndef __HIPCC_RTC__
#include <stdint.h>
#else
/* compiled at run time by hipRTC (the library's kernel specialiser) */
typedef __hip_internal::int32_t int32_t;
typedef __hip_internal::int64_t int64_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SDF_ABI_VERSION 12  /* 7: sdf_comm_create timeout, sdf_render_multi;
                                8: sdf_render_frames;
                                9: TILES carries shading terms (64-byte
                                   stream header), SDF_FORMAT_SHADE32F;
                                10: sdf_driver_config.batch (frames per
                                   ship); TILES base bits pixel by pixel
                                   (lane-major) instead of bit planes;
                                11: sdf_schedule_*, sdf_render_scheduled,
                                   sdf_tiles_decode_checked (SDF_TILES_BAD_*
                                   one byte each), sdf_validate bounds every
                                   length to 1e15;
                                12: sdf_params.samples (was reserved[0]):
                                   fused 2x2 / 4x4 supersampling in sdf_render
                                   and sdf_render_scheduled;
                                still 12: sdf_validate_lights and
                                   sdf_render_lights (SDF_MAX_LIGHTS,
                                   SDF_LIGHTS_COLOR) are additions -- no struct
                                   and no existing entry point changed, so the
                                   version stays; detect them by the symbol;
                                still 12: sdf_validate_materials and
                                   sdf_render_materials, additions likewise;
                                still 12: sdf_validate_reflect and
                                   sdf_render_reflect (sdf_reflect), additions
                                   likewise;
                                still 12: sdf_validate_env and sdf_render_env
                                   (sdf_environment, SDF_ENV_*), additions
                                   likewise;
                                still 12: sdf_validate_mesh, sdf_mesh_count,
                                   sdf_mesh_emit, sdf_mesh_workspace_bytes
                                   (sdf_grid, sdf_mesh_out), additions
                                   likewise;
                                still 12: sdf_validate_grad, sdf_sample_grad,
                                   sdf_grad_workspace_bytes (sdf_grad_out),
                                   additions likewise;
                                still 12: sdf_validate_points and
                                   sdf_shade_points (sdf_points,
                                   sdf_point_shade, SDF_POINTS_*), additions
                                   likewise;
                                still 12: sdf_validate_mesh_sharp and
                                   sdf_mesh_emit_sharp (sdf_mesh_sharp),
                                   additions likewise */

/* ---- status codes ------------------------------------------------------ */
#define SDF_OK               0
#define SDF_E_INVALID_ARG   -1  /* null pointer, bad size, bad enum value      */
#define SDF_E_UNSUPPORTED   -2  /* valid request this build cannot serve       */
#define SDF_E_HIP           -3  /* a HIP runtime call failed                   */
#define SDF_E_NO_DEVICE     -4  /* no gfx950 device visible                    */
#define SDF_E_COMM          -5  /* RCCL could not be loaded or a collective failed */
#define SDF_E_TIMEOUT       -6  /* the frame driver waited longer than its limit */

/* ---- scene description -------------------------------------------------- */
#define SDF_MAX_PRIMS 16

/* Primitive kinds.  Parameter layout in sdf_primitive.p[]:
 *   SPHERE     c.xyz, radius                       (voxel_fragment.frag:54-64)
 *   PLANE      n.xyz, h        sdf = dot(p, n) + h   (voxel_fragment.frag:66-71
 *                              is n = (0,1,0), h = 0: sdf = p.y)
 *   BOX        c.xyz, half.xyz                     (extension, parity unpinned)
 *   ROUND_BOX  c.xyz, half.xyz, r                  (extension)
 *   TORUS      c.xyz, R, r     ring in the xz plane (extension)
 *   CAPSULE    a.xyz, b.xyz, r                     (extension)
 *   CYLINDER   c.xyz, r, half_height, y-axis, capped (extension)            */
typedef enum {
  SDF_PRIM_SPHERE = 0,
  SDF_PRIM_PLANE = 1,
  SDF_PRIM_BOX = 2,
  SDF_PRIM_ROUND_BOX = 3,
  SDF_PRIM_TORUS = 4,
  SDF_PRIM_CAPSULE = 5,
  SDF_PRIM_CYLINDER = 6,
  SDF_PRIM_KIND_COUNT = 7
} sdf_prim_kind;

/* How primitive i combines with the running scene distance d (d starts at
 * +INF, voxel_fragment.frag:75).  UNION is GLSL `min(d, s)` exactly as
 * voxel_fragment.frag:77-78; the smooth forms use the polynomial smooth-min
 * with blend radius `k` (extension, see DESIGN.md "Scene spec").            */
typedef enum {
  SDF_OP_UNION = 0,
  SDF_OP_SMOOTH_UNION = 1,
  SDF_OP_SUBTRACT = 2,         /* max(d, -s)                                  */
  SDF_OP_INTERSECT = 3,        /* max(d, s)                                   */
  SDF_OP_SMOOTH_SUBTRACT = 4,
  SDF_OP_SMOOTH_INTERSECT = 5,
  SDF_OP_COUNT = 6
} sdf_csg_op;

typedef struct {
  int32_t kind;   /* sdf_prim_kind */
  int32_t op;     /* sdf_csg_op    */
  float k;        /* smooth blend radius (> 0 for SMOOTH_* ops)               */
  float reserved;
  float p[12];    /* kind-specific parameters, see above                      */
} sdf_primitive;  /* 64 bytes */

typedef enum {
  SDF_SCENE_PRIMITIVES = 0,    /* CSG list of prims[0..count)                 */
  SDF_SCENE_MANDELBULB = 1     /* power-8 Mandelbulb distance estimator        */
} sdf_scene_kind;

typedef struct {
  int32_t kind;                /* sdf_scene_kind                               */
  int32_t count;               /* number of primitives used (PRIMITIVES)       */
  sdf_primitive prims[SDF_MAX_PRIMS];
  /* MANDELBULB: world p -> local q = (p - center) / scale, DE(q) * scale.   */
  float bulb_center[3];
  float bulb_scale;
  int32_t bulb_iterations;     /* default 12                                   */
  float bulb_bailout;          /* default 2; (0, 2^32]                         */
  int32_t reserved[2];
} sdf_scene;

/* Camera: voxel_fragment.frag:26-30, :178-180, :191-192.                    */
typedef struct {
  float view[16];              /* V_mat uniform, column-major                  */
  float eye[3];                /* camera.pos before inverse(V_mat): (0,0.2,2)  */
  float fov_deg;               /* camera.fov = 60                              */
  float aspect;                /* AR uniform; <= 0 means width / height        */
  float pi;                    /* the shader's PI literal 3.1415925359f (a1)   */
} sdf_camera;

/* Light: voxel_fragment.frag:32-40, :182-184.                               */
typedef struct {
  float pos[3];                /* (5, 5, 0)                                    */
  float ambient;               /* light.amb = 0.1                              */
  float color[3];              /* light.col = 0.7: declared, never used by the
                                  shader (:183) nor by sdf_render; a factor on
                                  the light's diffuse and specular under
                                  sdf_render_lights with SDF_LIGHTS_COLOR      */
  float reserved;
} sdf_light;

/* Several lights (sdf_render_lights, "Lights" below) */
#define SDF_MAX_LIGHTS   8
#define SDF_LIGHTS_COLOR 0x1   /* light_flags: scale light i's diffuse and specular by lights[i].color */

/* Material: voxel_fragment.frag:42-49, :186-189.                            */
typedef struct {
  float amb[3];                /* (0, 0.2, 0.8)                                */
  float dif[3];                /* (0, 0.2, 0.8)                                */
  float ref[3];                /* (0.5, 0.5, 0.5)                              */
  float shininess;             /* 12                                           */
} sdf_material;

/* Mirror reflections (sdf_render_reflect, "Reflections" below) */
#define SDF_MAX_BOUNCES    4
#define SDF_REFLECT_WEIGHT 0x1      /* with layer >= 0: write W_layer instead of C_layer */
typedef struct {
  int32_t bounces;   /* 0 .. SDF_MAX_BOUNCES reflected rays per pixel               */
  float   strength;  /* finite; scales the blended ref into the mirror weight       */
  int32_t layer;     /* -1: the composite; 0 .. bounces: that layer alone            */
  int32_t flags;     /* SDF_REFLECT_WEIGHT                                          */
} sdf_reflect;       /* 16 bytes */

/* Environment (sdf_render_env, "Environment" below) */
#define SDF_ENV_SKY 0x1   /* a missed layer's colour is the sky along its ray      */
#define SDF_ENV_SUN 0x2   /* with SKY: a glow around sun_dir                        */
#define SDF_ENV_FOG 0x4   /* linear distance fog on every layer that is not sky     */
typedef struct {
  int32_t flags;          /* SDF_ENV_*; 0: sdf_render_reflect itself                 */
  float horizon[3];       /* SKY: the sky's colour at D.y = 0                        */
  float zenith[3];        /* SKY: straight up (D.y = 1)                              */
  float ground[3];        /* SKY: straight down (D.y = -1)                           */
  float sun_dir[3];       /* SUN: towards the sun, normalised by the caller          */
  float sun_color[3];     /* SUN: the glow's colour                                  */
  float sun_exponent;     /* SUN: finite, >= 1; the glow is max(D . sun_dir, 0)^it   */
  float fog_color[3];     /* FOG                                                     */
  float fog_start;        /* FOG: no fog up to this march distance                   */
  float fog_end;          /* FOG: all fog from here on; fog_end - fog_start > 0      */
  int32_t reserved[2];
} sdf_environment;        /* 96 bytes */

/* Query outputs (sdf_trace, sdf_trace_camera; "Queries" below): device
 * pointers, one entry per ray.  Any may be NULL, at least one is not.        */
typedef struct {
  float*   t;       /* n floats:  the march's distance d                        */
  int32_t* steps;   /* n int32:   the march's iteration count                   */
  float*   normal;  /* 3n floats, packed xyz; NULL: no normal is evaluated      */
  int32_t* prim;    /* n int32:   the primitive that owns the hit; NULL: none   */
} sdf_hits;         /* 32 bytes */

/* Caller-supplied rays (sdf_render_rays; "Rays" below): device pointers.     */
#define SDF_RAYS_UNIT 0x1   /* dirs are unit vectors, used as given */
typedef struct {
  const float* origins;   /* device, n x 3 packed fp32 */
  const float* dirs;      /* device, n x 3 packed fp32 */
  int64_t n;
  int32_t flags;          /* SDF_RAYS_* */
  int32_t reserved;
} sdf_rays;               /* 32 bytes */

/* Shading at caller-supplied points (sdf_shade_points; "Points" below):
 * device pointers. */
#define SDF_POINTS_EYE 0x1      /* eye is set: the specular term is evaluated */
typedef struct {
  const float* points;    /* device, n x 3 packed fp32 */
  const float* normals;   /* device, n x 3 packed fp32, optional: used as given */
  int64_t n;
  float eye[3];           /* with SDF_POINTS_EYE */
  float lift;             /* finite, >= 0: P = Q + N lift */
  int32_t flags;          /* SDF_POINTS_* */
  int32_t reserved;       /* 0 */
} sdf_points;             /* 48 bytes */
typedef struct {
  float*   rgba;      /* n x 4: the colour sum, alpha 1; 16-byte aligned */
  float*   ao;        /* n: the occlusion term */
  float*   shadow;    /* n x nlights: light i's soft-shadow factor sh_i */
  float*   material;  /* n x 9: the blended amb, dif, ref */
  int32_t* steps;     /* n x nlights: light i's shadow-march count */
} sdf_point_shade;    /* 40 bytes; any pointer may be NULL, at least one is not */

/* Isosurface meshes (sdf_mesh_count, sdf_mesh_emit; "Meshes" below) */
#define SDF_MESH_DENSE 0x1          /* evaluate every brick: no distance-bound skipping (cross-check) */
typedef struct {
  float origin[3];                  /* lattice point (0,0,0) */
  float cell[3];                    /* cell size per axis, finite, > 0 */
  int32_t n[3];                     /* cells per axis, >= 1; (n0+1)(n1+1)(n2+1) <= 2^30 */
  float iso;                        /* the level set extracted: f(p) = iso (0: the surface; > 0: an offset shell) */
  int32_t flags;                    /* SDF_MESH_* */
  int32_t reserved;                 /* 0 */
} sdf_grid;                         /* 48 bytes */
typedef struct {
  float*   verts;   int64_t max_verts;  /* device, 3 floats per vertex */
  int32_t* tris;    int64_t max_tris;   /* device, 3 vertex indices per triangle */
  float*   normal;                      /* device, optional, 3 per vertex */
  int32_t* prim;                        /* device, optional, 1 per vertex */
} sdf_mesh_out;                         /* 48 bytes */
/* Sharp-feature vertices (sdf_mesh_emit_sharp; "Sharp meshes" below) */
typedef struct {
  int32_t refine;      /* 0 .. 8: regula-falsi steps per crossing edge      */
  int32_t iterations;  /* 0 .. 64: descent steps of the vertex fit          */
  int32_t flags;       /* 0                                                 */
  int32_t reserved;    /* 0                                                 */
} sdf_mesh_sharp;      /* 16 bytes */

/* Gradients (sdf_sample_grad; "Gradients" below) */
typedef struct {
  float* dist;         /* device, n, optional: f(p_i)                                   */
  float* grad_points;  /* device, 3n packed, optional: g_i * df/dp at p_i               */
  float* grad_prims;   /* device, SDF_MAX_PRIMS * 16 floats, optional (layout below)    */
} sdf_grad_out;        /* 24 bytes; at least one pointer non-NULL */

/* Measures (sdf_measure; "Measures" below) */
#define SDF_MEASURE_OWNERS 0x1      /* rows 1 + k: the inside samples primitive k owns */
#define SDF_MEASURE_SLOTS  16       /* int64 per row */
#define SDF_MEASURE_ROWS   (1 + SDF_MAX_PRIMS)

/* Render flags */
#define SDF_FLAG_SHADOW    0x1  /* soft shadow march (voxel_fragment.frag:205) */
#define SDF_FLAG_AO         0x2  /* ambient occlusion (extension)               */

typedef enum {
  SDF_NORMAL_CENTRAL = 0,      /* 6-tap central differences (:134-155)         */
  SDF_NORMAL_TETRA = 1         /* 4-tap tetrahedral differences (extension)    */
} sdf_normal_mode;

typedef enum {
  SDF_PRECISION_EXACT = 0,     /* IEEE div/sqrt, no FMA contraction: bit-level
                                  restatement of the shader arithmetic         */
  SDF_PRECISION_FAST = 1       /* hardware sqrt/rcp, FMA contraction           */
} sdf_precision;

typedef struct {
  int32_t width, height;       /* framebuffer size (main.cpp:4-5: 800 x 600)   */
  int32_t max_steps;           /* MAX_STEPS = 100 (both marches, :17)          */
  float max_dist;              /* MAX_DISTANCE = 100 (:18)                     */
  float eps;                   /* EPSILON = 0.01 (:19)                         */
  float shadow_k;              /* 10 (:205)                                    */
  float normal_eps;            /* DX/DY/DZ offset = EPSILON (:21-23)           */
  float shadow_offset;         /* P + N*2*EPSILON: 2 (:205)                    */
  int32_t flags;               /* SDF_FLAG_*; reference = SDF_FLAG_SHADOW      */
  int32_t normal_mode;         /* sdf_normal_mode; reference = CENTRAL          */
  int32_t ao_taps;             /* AO samples (5 when SDF_FLAG_AO)              */
  float ao_step;               /* AO: h_i = ao_base + ao_step * i / (taps-1)   */
  float ao_base;
  float ao_falloff;            /* per-tap weight decay                         */
  float ao_strength;           /* ao = clamp(1 - strength * occ, 0, 1)         */
  int32_t precision;           /* sdf_precision                                */
  int32_t dispatch;            /* sdf_dispatch (AUTO: compile-time scene
                                  variant when one matches the scene)         */
  int32_t output_format;       /* sdf_format of the framebuffer written       */
  int32_t samples;             /* sub-samples per axis: 0 or 1 one sample per
                                  pixel, 2 or 4 supersampling (below); anything
                                  else is SDF_E_INVALID_ARG                    */
  int32_t reserved[1];
} sdf_params;

/* Supersampling (sdf_params.samples = S, 2 or 4; ABI 12).  The pixel -> quad
 * map is ((2x+1)/W - 1, (2y+1)/H - 1), so the S x S sub-sample grid of a
 * W x H frame is exactly the pixel grid of the S W x S H frame (and the
 * default aspect (float)(S W) / (float)(S H) is the same float as W / H):
 *   - sub-sample (i, j) of output pixel (x, y) is pixel (S x + i, S y + j) of
 *     the S W x S H frame; its colour c[i][j] is what sdf_render writes for
 *     that pixel as RGBA32F with samples = 0, in the request's precision.
 *   - resolve, per channel R, G, B, in fp32 round-to-nearest without fused
 *     multiply-add, a balanced pairwise tree, first along x, then along y,
 *     left / lower operand first:
 *       S = 2   h_j = c[0][j] + c[1][j];   out = (h_0 + h_1) * 0.25f
 *       S = 4   a_j = (c[0][j] + c[1][j]) + (c[2][j] + c[3][j]);
 *               out = ((a_0 + a_1) + (a_2 + a_3)) * 0.0625f
 *     alpha is 1; denormals are kept.  tests/ssaa_ref.py states it in NumPy.
 *   - the output format's conversion (RGBA16F, RGBA8, RGB32F) is applied to
 *     the resolved colour exactly as to a pixel's colour.  `rgba` holds the
 *     W x H output (owned rows x W): no S W x S H buffer exists.
 *   - limits: S * width <= 65536 and S * height <= 65536 (and S * block_rows
 *     of a tiling fits int32), else SDF_E_INVALID_ARG; SDF_FORMAT_TILES and
 *     SDF_FORMAT_SHADE32F are SDF_E_UNSUPPORTED (shading terms do not average
 *     to the colour).
 *   - a tiling refers to output rows: the render equals the S W x S H render
 *     under the same tiling with block_rows * S, resolved; packed rows and
 *     SDF_TILING_FRAME_ROWS work as with one sample.
 *   - `steps`, when non-null, receives the sub-samples' counts: S * rows x
 *     S * width int2, laid out as the steps buffer of the S W x S H render
 *     under that scaled tiling (S * height rows with SDF_TILING_FRAME_ROWS);
 *     sdf_heatmap works on it unchanged.
 *   - sdf_render_scheduled serves it with a schedule created for S x the
 *     owned rows (the kernel's 8-row cost blocks are sub-sample rows, so S *
 *     rows <= 4096); a schedule of any other row count renders in launch
 *     order, as for any render it does not fit.
 *   - sdf_render_frames, sdf_render_multi and sdf_driver_create (at any world
 *     size) return SDF_E_UNSUPPORTED for samples > 1, decided before any
 *     device call: their TILES streams and the persistent frames kernel carry
 *     no resolve.  Jittered or rotated grids, filters other than the box and
 *     samples = 8 are not offered. */

/* Lights (sdf_render_lights: L = nlights point lights, 1 .. SDF_MAX_LIGHTS,
 * with light_flags).  The frame is defined from what sdf_render gives with one
 * light at a time, so it can be checked bit for bit (tests/lights_ref.py
 * states it in NumPy):
 *   - geometry: the primary march, the hit point P, the normal N and the
 *     ambient-occlusion term ao of a pixel are those of sdf_render; they do
 *     not depend on the light.
 *   - per-light terms: (dif_i, x_i) of light i are bit for bit channels 1 and
 *     2 of what sdf_render writes as SDF_FORMAT_SHADE32F with light =
 *     lights[i], in the request's precision (dif = clamp(N.L, 0, 1) * shadow,
 *     x = max(N.H, 0)); spec_i = x_i ^ shininess as sdf_render forms it in
 *     that precision (exact: fp64 pow rounded to fp32 once; fast: exp2(shin *
 *     log2(x)) with the hardware's v_exp_f32 / v_log_f32 and one fp32 product).
 *   - ambient: la = the fp32 sum of lights[i].ambient in index order (one
 *     light: its own value); lam[c] = RN(la * material.amb[c]).  The ambient
 *     term is never coloured.
 *   - colour sum, per channel c = R, G, B, in fp32 round-to-nearest, lights
 *     in index order, never reassociated:
 *       acc = RN(lam[c] * ao)
 *       for i in 0 .. L-1:
 *         with SDF_LIGHTS_COLOR  d = RN(dif_i * lights[i].color[c]),
 *                                s = RN(spec_i * lights[i].color[c])
 *                                (plain products, never fused)
 *         otherwise              d = dif_i, s = spec_i
 *         exact precision  acc = RN(RN(acc + RN(d * mat.dif[c])) + RN(s * mat.ref[c]))
 *         fast precision   acc = fma(s, mat.ref[c], fma(d, mat.dif[c], acc))
 *                          (each fma rounded once)
 *     out[c] = acc, alpha is 1.  For one light without the flag this is
 *     sdf_render's colour exactly.  A colour is an arbitrary finite factor
 *     (negative ones included); lights[i].color is ignored without the flag.
 *   - steps, when non-null, receives (primary, sum over i of shadow_i) per
 *     pixel, shadow_i being light i's count in its own sdf_render; as in
 *     sdf_render every shadow march then runs to the reference's break.
 *     sdf_heatmap works on the result unchanged.
 *   - nlights = 1 with light_flags = 0 is sdf_render / sdf_render_scheduled
 *     itself: the same kernels, every format, the same bits.
 *   - output conversion (RGBA16F, RGBA8, RGB32F), tilings, SDF_TILING_FRAME_ROWS
 *     and schedules work as in sdf_render / sdf_render_scheduled.  With
 *     samples = 2 or 4 a sub-sample's colour is the L-light colour of its pixel
 *     of the S W x S H frame, resolved as under "Supersampling".
 *   - SDF_E_INVALID_ARG (sdf_validate_lights, and sdf_render_lights before any
 *     device call): lights NULL; nlights < 1 or > SDF_MAX_LIGHTS; light_flags
 *     bits other than SDF_LIGHTS_COLOR; a light whose position fails
 *     sdf_validate's checks of its one light (finite, |.| <= 1e15); with
 *     SDF_LIGHTS_COLOR a non-finite colour component.  Everything else is
 *     validated by sdf_validate with lights[0].
 *   - SDF_E_UNSUPPORTED: SDF_FORMAT_TILES and SDF_FORMAT_SHADE32F with
 *     nlights > 1 or SDF_LIGHTS_COLOR (a stream carries one light's terms).
 *   - sdf_render_frames, sdf_render_multi and the frame driver keep their one
 *     light.  Directional and spot lights, per-light shadow switches,
 *     attenuation and more than SDF_MAX_LIGHTS lights are not offered. */

/* Materials (sdf_render_materials: materials[i] belongs to scene->prims[i];
 * nmaterials = scene->count for a primitive scene, 1 for a Mandelbulb).  The
 * frame is sdf_render_lights's with the one material replaced, per pixel, by
 * a blend of the primitives' materials that follows the scene's CSG fold, so
 * it can be checked bit for bit (tests/materials_ref.c states it in C over
 * the CPU oracle):
 *   - geometry and lights: the primary march, P, N, ao and every light's
 *     (dif_i, x_i) are exactly those of sdf_render_lights; they do not depend
 *     on the materials.
 *   - the material fold: after the march the primitive list is evaluated once
 *     more at P, every primitive, in list order, carrying the scene fold's
 *     running distance d (+INF before primitive 0) and a running material m
 *     of 9 components (amb, dif, ref), which starts as materials[0].  For
 *     primitive i with value v = s_i(P) and blend radius k, (a, b) are the
 *     arguments the scene fold hands to min / smooth-min:
 *       UNION, SMOOTH_UNION           (a, b) = ( d,  v)
 *       SUBTRACT, SMOOTH_SUBTRACT     (a, b) = (-d,  v)
 *       INTERSECT, SMOOTH_INTERSECT   (a, b) = (-d, -v)
 *     hard operators: t = (b < a) ? 1 : 0 -- on a tie the earlier owner stays,
 *     and the cutter of a subtraction owns the surface it carves;
 *     smooth operators: h = max(k - |a - b|, 0) / k, the smooth-min's own h
 *     (exact precision: these fp32 operations with an IEEE division; fast
 *     precision: the clamped fma(-|a - b|, 1/k, 1) of its smooth-min),
 *     q = RN(RN(h h) 0.5), t = (b < a) ? RN(1 - q) : q;
 *     each of the 9 components: unchanged for t = 0, materials[i]'s for t = 1,
 *     else  exact precision  m = RN(m + RN(t RN(M_i - m)))   (never fused)
 *           fast precision   m = fma(t, RN(M_i - m), m);
 *     then d advances by the scene fold's combine.  There is no miss branch
 *     (the reference has none): the fold runs at whatever P the march ended
 *     on.  With d = +-INF, h = 0 and t is 0 or 1: no NaN arises.
 *   - colour: the "Lights" colour sum with material.amb / dif / ref[c]
 *     replaced by the pixel's blended components, lam[c] = RN(la amb_px[c]).
 *   - shininess stays frame-wide: every entry must carry the bits of
 *     materials[0].shininess (SDF_E_UNSUPPORTED otherwise).
 *   - if the amb, dif and ref of all entries are byte-identical (always with
 *     nmaterials = 1, so for a Mandelbulb) the call is sdf_render_lights with
 *     materials[0]: the same kernels, every format, the same bits.
 *   - output conversion, tilings, SDF_TILING_FRAME_ROWS, schedules, samples =
 *     2 / 4 and `steps` work as in sdf_render_lights (the fold is not counted
 *     in steps; a sub-sample's colour is its pixel's of the S W x S H frame).
 *   - SDF_E_INVALID_ARG (sdf_validate_materials, and sdf_render_materials
 *     before any device call): materials NULL; nmaterials not the scene's
 *     count (1 for a Mandelbulb); anything sdf_validate_lights rejects
 *     (sdf_validate checks a material's presence only, so an entry cannot
 *     fail on its own).
 *   - SDF_E_UNSUPPORTED: entries whose shininess differs; SDF_FORMAT_TILES or
 *     SDF_FORMAT_SHADE32F with distinct materials (a stream carries one
 *     material's constants).
 *   - sdf_render_frames, sdf_render_multi and the frame driver keep their one
 *     material.  Textures, procedural patterns and a shininess per primitive
 *     are not offered. */

/* Reflections (sdf_render_reflect: the "Materials" frame with up to
 * SDF_MAX_BOUNCES mirror bounces per pixel; everything except `reflect` means
 * what it means in sdf_render_materials; tests/reflect_ref.c walks the same
 * path with the CPU oracle's own shade_pixel):
 *   - layers: a pixel's path is a sequence of rays (O_j, D_j), j = 0, 1, ...
 *     (O_0, D_0) is the camera position and the pixel's ray exactly as
 *     sdf_render forms them.  Layer j is the "Materials" pipeline run for a
 *     fragment whose eye is O_j and whose ray is D_j: the primary march from
 *     O_j along D_j gives d_j and P_j = O_j + D_j d_j; N_j and ao_j are taken
 *     at P_j; the material fold at P_j gives amb_j, dif_j, ref_j (materials[0]'s
 *     for a Mandelbulb); every light's (dif_i, x_i) uses view = normalize(O_j -
 *     P_j) and a shadow march from P_j; the colour sum in the precision's
 *     operation sequence gives C_j.  Layer 0 is sdf_render_materials's pixel,
 *     bit for bit, in both precisions.
 *   - next ray (fp32): nd = dot(N_j, D_j), the left-to-right sum of three
 *     products; s = 2 nd; R.c = D_j.c - s N_j.c; D_(j+1) = normalize(R);
 *     O_(j+1) = P_j + N_j shadow_offset eps, evaluated as the shadow march's
 *     origin is ((P.c + N.c * shadow_offset * eps), left to right).  Exact
 *     precision rounds every operation once and fuses nothing, normalize with
 *     IEEE sqrt and division; fast precision is free to contract.  There is no
 *     branch on the sign of nd.
 *   - weights: W_0 = (1, 1, 1); k_j[c] = RN(strength ref_j[c]);
 *     W_(j+1)[c] = RN(W_j[c] k_j[c]), in both precisions.
 *   - end of a path: layer j is the pixel's last when j = bounces, or its
 *     primary march ended with d_j > max_dist (a miss: nothing is reflected off
 *     the far point), or all three components of W_(j+1) compare equal to 0 (a
 *     matte surface spawns no ray).  Nothing else ends a path: a march that
 *     runs out of steps, or a NaN normal, goes on as the arithmetic says.
 *   - composite (layer = -1): acc = C_0, then for j = 1 .. last in order
 *       exact precision  acc[c] = RN(acc[c] + RN(W_j[c] C_j[c]))
 *       fast precision   acc[c] = fma(W_j[c], C_j[c], acc[c])
 *     and the pixel is (acc, 1).  `steps`, when non-null, receives (sum_j
 *     primary_j, sum_j sum_i shadow_(j,i)) over the layers traced; as in
 *     sdf_render every shadow march then runs to the reference's break.
 *   - one layer (layer = j >= 0, a render pass): the pixel is (C_j, 1), with
 *     SDF_REFLECT_WEIGHT (W_j, 1); `steps` receives layer j's own counts; a
 *     pixel whose path ended before layer j gets (0, 0, 0, 1) and (0, 0).
 *   - bounces = 0 with layer -1 or 0 and no weight flag IS
 *     sdf_render_materials: the same kernels, every format, the same bits.
 *   - with bounces >= 1 (or the weight flag) SDF_FORMAT_TILES and
 *     SDF_FORMAT_SHADE32F are SDF_E_UNSUPPORTED; RGBA16F, RGBA8 and RGB32F
 *     convert the output colour as usual.
 *   - tilings, SDF_TILING_FRAME_ROWS and schedules work as in
 *     sdf_render_materials; with samples = 2 or 4 a sub-sample's colour is its
 *     pixel's of the S W x S H frame, resolved as under "Supersampling"; the
 *     shininess stays frame-wide.
 *   - SDF_E_INVALID_ARG (sdf_validate_reflect, and sdf_render_reflect before
 *     any device call): reflect NULL; bounces outside 0 .. SDF_MAX_BOUNCES;
 *     layer outside -1 .. bounces; unknown flag bits, or the weight flag with
 *     layer = -1; a non-finite strength; with bounces >= 1 a non-finite amb,
 *     dif or ref component; anything sdf_validate_materials rejects (its
 *     SDF_E_UNSUPPORTED cases stay SDF_E_UNSUPPORTED).
 *   - refraction, Fresnel weighting, glossy reflection and a background colour
 *     for misses are not offered; sdf_render_frames, sdf_render_multi and the
 *     frame driver keep their one layer. */

/* Environment (sdf_render_env: the "Reflections" frame with a sky for the rays
 * that leave the scene and linear distance fog; everything except `env` means
 * what it means in sdf_render_reflect; layers, rays (O_j, D_j), d_j, C_j, k_j
 * and W_j are those of "Reflections"; tests/env_ref.py states it in NumPy over
 * the planes of that block's reference):
 *   - miss: layer j is a miss when d_j > max_dist, the comparison that already
 *     ends a path.  A NaN d_j is not a miss.
 *   - sky (SDF_ENV_SKY): the colour of a missed layer is sky(D_j) instead of
 *     C_j, and nothing after the primary march is evaluated for that layer: no
 *     normal, no ambient occlusion, no material fold, no light.  u = D_j.y, up
 *     = !(u < 0), t = clamp(up ? u : -u, 0, 1) with the GLSL selects (max(x, 0)
 *     = x < 0 ? 0 : x, min(x, 1) = 1 < x ? 1 : x), B = up ? zenith : ground, and
 *     sky[c] = mix(horizon[c], B[c], t) with the "Materials" mix: horizon[c]
 *     unchanged for t = 0, B[c] for t = 1, else
 *       exact precision  RN(horizon[c] + RN(t RN(B[c] - horizon[c])))
 *       fast precision   fma(t, RN(B[c] - horizon[c]), horizon[c])
 *   - sun (SDF_ENV_SUN, with SKY): g = max(dot(D_j, sun_dir), 0), the dot
 *     product the left-to-right sum of three rounded products in both
 *     precisions, sun_dir as given (the caller normalises it); glow = pow(g,
 *     sun_exponent) as the specular term's power is taken (exact: fp64 pow
 *     rounded once; fast: exp2(sun_exponent log2(g)) in hardware); then
 *       exact precision  sky[c] = RN(sky[c] + RN(glow sun_color[c]))
 *       fast precision   sky[c] = fma(glow, sun_color[c], sky[c])
 *   - fog (SDF_ENV_FOG) applies to every layer the sky did not replace: every
 *     hit layer, and every missed layer when SKY is off.  f_j = clamp((fog_end -
 *     d_j) / RN(fog_end - fog_start), 0, 1), d_j the layer's own march distance
 *     from O_j; exact precision rounds every operation once with an IEEE
 *     division, fast precision multiplies by the host's RN(1 / RN(fog_end -
 *     fog_start)).  C'_j[c] = mix(fog_color[c], C_j[c], f_j) with the mix above,
 *     so f = 1 leaves the bits of C_j and f = 0 gives the fog colour's.  What
 *     lies behind a fogged surface is attenuated too: W_(j+1)[c] = RN(RN(W_j[c]
 *     k_j[c]) f_j) in both precisions (without the flag there is no second
 *     product), and "all three components of W_(j+1) compare equal to 0" now
 *     also ends a path that is fully in fog.
 *   - composite, passes, steps: "Reflections"' composite with C'_j (or the
 *     sky) in place of C_j and the weights above; layer = j writes that
 *     layer's final colour, SDF_REFLECT_WEIGHT the weight above; `steps` as
 *     there, except that under SKY a missed layer counts (primary_j, 0).  Alpha
 *     is 1; NaNs propagate as the arithmetic says.
 *   - env NULL or flags = 0 IS sdf_render_reflect: the same kernels, every
 *     format, the same bits (so with bounces = 0 sdf_render_materials, and so
 *     on down).  With a flag set bounces = 0 is legal: one layer through the
 *     env kernel.
 *   - with a flag set SDF_FORMAT_TILES and SDF_FORMAT_SHADE32F are
 *     SDF_E_UNSUPPORTED; RGBA16F, RGBA8 and RGB32F convert the colour as usual;
 *     tilings, SDF_TILING_FRAME_ROWS, schedules and samples = 2 or 4 work as in
 *     "Reflections".
 *   - SDF_E_INVALID_ARG (sdf_validate_env, and sdf_render_env before any
 *     device call): unknown flag bits; SUN without SKY; with SKY a non-finite
 *     horizon, zenith or ground component; with SUN a non-finite sun_dir or
 *     sun_color component or a sun_exponent that is not finite and >= 1; with
 *     FOG a non-finite fog_color, fog_start or fog_end, or den = RN(fog_end -
 *     fog_start) not greater than 0, or den or RN(1 / den) not finite (a range
 *     wider than FLT_MAX or of at most 2^-128: the factor could not be
 *     formed in both precisions); anything sdf_validate_reflect rejects (its
 *     SDF_E_UNSUPPORTED cases stay SDF_E_UNSUPPORTED).  Fields of a feature
 *     whose flag is off are ignored.
 *   - exponential fog (it needs a correctly rounded exp), environment maps or
 *     textures, per-channel fog, and an environment in sdf_render_frames,
 *     sdf_render_multi or the frame driver are not offered. */

/* Queries (sdf_trace, sdf_trace_camera, sdf_sample: what a render computes on
 * the way to a colour, asked of the scene directly -- picking, depth, normal
 * and primitive-id maps, rays of the caller's own camera model, the distance
 * field on a set of points.  `origins`, `dirs` and `points` are device arrays
 * of n x 3 packed fp32; every output is defined from the CPU oracle's point
 * probes, so it can be checked bit for bit (tests/query_ref.py states it in
 * NumPy).  Exact precision rounds every operation once and fuses nothing;
 * fast precision uses the hardware reciprocal square root and may contract,
 * as everywhere else:
 *   - ray i of sdf_trace: O = origins[i] as given; D = normalize(dirs[i]) with
 *     the precision's own normalize (exact: the left-to-right sum of three
 *     rounded products, an IEEE square root and three IEEE divisions, as
 *     "Reflections" forms D_(j+1)).  The kernel normalises instead of trusting
 *     the caller: the kernels' culling is proven for |D| <= 1 + 2^-22.
 *   - march: sdf_render's primary march from O along D with params->max_steps,
 *     max_dist and eps; its distance d goes to `t`, its iteration count to
 *     `steps`.
 *   - miss: d > max_dist, the comparison that ends a reflect path (a NaN d is
 *     not a miss): `normal` is (0, 0, 0), `prim` is -1, and nothing after the
 *     march is evaluated for that ray, as for a missed layer under a sky.
 *   - hit: P = O + D d as the render forms it; `normal` is N at P with
 *     params->normal_mode and normal_eps.
 *   - `prim` is the owner fold at P: the primitive list is evaluated once
 *     more, every primitive, in list order, carrying the scene fold's running
 *     d (+INF before primitive 0) and an owner w that starts at 0.  For
 *     primitive i, (a, b) are the pair "Materials" defines for its operator;
 *     w becomes i when b < a, for hard and smooth operators alike (for a
 *     smooth one that is the side with the larger blend weight: t = (b < a) ?
 *     1 - q : q with q <= 1/2); then d advances by the scene fold's combine.
 *     A tie or a NaN keeps the earlier owner.  A Mandelbulb always gives 0.
 *   - sdf_trace_camera: entry y * width + x is the ray (O_0, D_0) of pixel
 *     (x, y) exactly as sdf_render forms it (the default aspect applies, no
 *     second normalisation), so its `steps` equal sdf_render's steps[..][0]
 *     for the same scene, camera and params, whatever the flags.  The whole
 *     frame, one ray per pixel: params->samples > 1 is SDF_E_UNSUPPORTED, and
 *     there is no tiling.
 *   - sdf_sample: dist[i] is the scene SDF at points[i]; `normal` (optional)
 *     the normal there with params->normal_mode and normal_eps.  There is no
 *     march and no miss.
 *   - params: max_steps, max_dist, eps, normal_eps, normal_mode, precision and
 *     dispatch are used (sdf_trace_camera: width and height too); every other
 *     field is ignored -- a copy with those fields at sdf_defaults' values is
 *     what is validated.  sdf_validate_query is that check with sdf_validate's
 *     scene checks; it makes no device call.
 *   - dispatch follows sdf_render's: a built-in variant when the scene matches
 *     one, under SDF_DISPATCH_AUTO a run-time specialised query kernel for any
 *     other primitive list (counted by sdf_jit_count; the generic kernel with
 *     SDF3D_JIT=0), GENERIC and UNCULLED as there.  In fast precision the
 *     kernels need not agree to the bit.
 *   - SDF_E_INVALID_ARG, decided before any device call: scene, params or hits
 *     NULL; every output pointer NULL; NULL inputs with n > 0; n < 0 or n >
 *     2^30; anything the validator rejects.  n = 0 is SDF_OK: nothing is
 *     launched, no buffer is touched and no device is needed.
 *   - a zero or non-finite direction (a direction whose length is 0, INF or
 *     NaN: normalize gives D NaN components) marches as the arithmetic of the
 *     scene spec says, whose min, max and clamp are the GLSL selects (min(x, y)
 *     = y < x ? y : x, max(x, y) = x < y ? y : x): a select keeps or drops a
 *     NaN by its position, so a list of hard unions gives t = +INF after one
 *     step (a miss), a smooth union t = NaN with steps = max_steps (a NaN d is
 *     not a miss: normal NaN, prim 0), exactly as the CPU oracle does.  The
 *     kernels route such a ray through a restatement of the scene spec with
 *     the selects; it costs the other rays of a call nothing.
 *   - device data: coordinates (origins, points) must be finite and at most
 *     1e15 in magnitude, what sdf_validate demands of the camera eye: the
 *     caller's duty, device data cannot be validated on the host.  Outside
 *     that range the values are unspecified, but the kernel still terminates:
 *     every loop is bounded by max_steps, and no address or index depends on
 *     ray data.
 *   - asynchronous on `stream`.  SDF_ABI_VERSION stays 12: detect the entry
 *     points by the symbol.
 *   - per-ray distance limits, sorting or compacting rays, tilings and several
 *     devices are not offered; gradients are sdf_sample_grad ("Gradients"),
 *     occlusion, soft shadows and shaded colours at points sdf_shade_points
 *     ("Points"). */

/* Rays (sdf_render_rays: the shading pipeline of "Environment" on rays of the
 * caller's own -- an orthographic view, a fisheye, a panorama, a stereo pair,
 * lens distortion, thin-lens jitter, secondary rays; sdf_camera_rays: the
 * render's own rays as a starting point).  The rendering counterpart of
 * "Queries": entry i of the outputs belongs to ray i.
 *   - ray i has O = origins[i] as given.  Without SDF_RAYS_UNIT, D =
 *     normalize(dirs[i]) in the precision's own normalize, as "Queries" defines
 *     it for sdf_trace.  With SDF_RAYS_UNIT, D = dirs[i] unchanged: the caller
 *     promises |D| <= 1 + 2^-22, the bound the kernels' cached-gap culling is
 *     proven for (every D of sdf_camera_rays keeps it).  Outside that bound the
 *     values are unspecified, but the kernel still terminates: every loop is
 *     bounded by max_steps, and no address depends on ray data.
 *   - entry i of `rgba` is the "Environment" pixel whose (O_0, D_0) is (O, D);
 *     with env NULL or env->flags 0 the "Reflections" pixel; with reflect NULL
 *     that of bounces 0 with layer -1.  Layers, weights, the composite, the
 *     `layer` passes, SDF_REFLECT_WEIGHT, sky, sun and fog carry over word for
 *     word; the view vector of layer 0 is normalize(O - P_0).  In exact
 *     precision the rays of sdf_camera_rays under SDF_RAYS_UNIT therefore give
 *     sdf_render_env's frame bit for bit.
 *   - `steps`, when non-null, is n int2 with the sums those blocks define; as
 *     there, every shadow march then runs to the reference's break.
 *   - inactive rays: a ray whose D has a component that is not finite -- without
 *     SDF_RAYS_UNIT a direction whose normalize has one (a length of 0 or NaN,
 *     an infinite component), with SDF_RAYS_UNIT such a component as given.
 *     Nothing is marched for it; its output is all-zero, alpha included, so
 *     alpha 0 is a mask the caller can use (outside a fisheye's image circle,
 *     say); its steps are (0, 0).  RGB32F has no alpha and writes (0, 0, 0).
 *     This differs on purpose from sdf_trace, which marches such a ray as the
 *     oracle does: a shaded NaN path has no reference meaning, and a mask is
 *     what a custom camera needs.
 *   - params: every shading and march field is used.  width, height and samples
 *     play no part: a copy with width / height at sdf_defaults' values is what
 *     is validated, together with a default camera.  samples > 1 is
 *     SDF_E_UNSUPPORTED: the caller supplies more rays and averages.
 *   - formats: RGBA32F, RGBA16F, RGBA8 and RGB32F, n packed pixels.  TILES and
 *     SHADE32F are SDF_E_UNSUPPORTED.  There is no tiling, no schedule and no
 *     multi-device form.
 *   - dispatch follows sdf_render's: a built-in variant when the scene matches
 *     one, under SDF_DISPATCH_AUTO a run-time specialised rays kernel for any
 *     other primitive list (counted by sdf_jit_count; the generic kernel with
 *     SDF3D_JIT=0), GENERIC and UNCULLED as there.
 *   - SDF_E_INVALID_ARG, decided before any device call: rays, scene or params
 *     NULL; unknown ray flag bits; n < 0 or n > 2^30; NULL origins, dirs or rgba
 *     with n > 0; anything sdf_validate_env rejects for these lights,
 *     materials, reflect and env (its SDF_E_UNSUPPORTED cases stay
 *     SDF_E_UNSUPPORTED).  sdf_validate_rays is that check without the buffers;
 *     it makes no device call.  n = 0 is SDF_OK: nothing is launched, no buffer
 *     is touched and no device is needed.
 *   - device data: origins must be finite and at most 1e15 in magnitude, the
 *     caller's duty as under "Queries".
 *   - a wave shades 64 consecutive rays: order the rays in coherent groups of
 *     64 (an 8 x 8 tile of an image, say); rays of one wave that go different
 *     ways wait for each other.
 *   - sdf_camera_rays: entry y * width + x of `origins` / `dirs` (device,
 *     width * height x 3 packed fp32) is (O_0, D_0) of pixel (x, y) as sdf_render
 *     forms them in params->precision; the default aspect applies.  Either
 *     output may be NULL, not both.  It uses width, height and precision and is
 *     validated like sdf_trace_camera; samples > 1 is SDF_E_UNSUPPORTED.
 *   - asynchronous on `stream`.  SDF_ABI_VERSION stays 12: detect the entry
 *     points by the symbol.
 *   - supersampling, tilings and schedules, frame sequences and several
 *     devices, TILES and SHADE32F output, per-ray distance limits, sorting or
 *     compacting rays and a NaN-marching path for shaded rays are not offered. */

/* Meshes (sdf_mesh_count, sdf_mesh_emit: the level set f(p) = iso of the scene
 * inside a regular grid, as an indexed triangle mesh -- export, printing,
 * collision, other tools.  Surface nets: one vertex per cell the surface passes
 * through, one quad per lattice edge it crosses.  Every output is defined from
 * what sdf_sample returns, so exact precision can be checked bit for bit
 * (tests/mesh_ref.py states it in NumPy over the CPU oracle).  Axes c = 0, 1, 2;
 * for an axis a, u = (a + 1) mod 3 and v = (a + 2) mod 3.  Exact precision rounds
 * every operation once and fuses nothing, divisions are IEEE; fast precision
 * may contract and use the hardware reciprocal.  Non-finite values propagate as
 * the arithmetic says:
 *   - two calls: sdf_mesh_count classifies the grid, fills `workspace` and
 *     writes counts[0] vertices, counts[1] triangles, counts[2] bricks whose
 *     lattice was evaluated, counts[3] bricks in all (device, 4 int64).  The
 *     caller reads them, sizes the buffers, and hands sdf_mesh_emit the same
 *     scene, params, grid and untouched workspace, ordered after the count;
 *     emit writes the mesh.  Every store of emit is guarded: vertex v (its
 *     normal, its prim) is written only if v < max_verts, triangle t only if t <
 *     max_tris, so an undersized buffer or a stale workspace cannot make emit
 *     write outside the caller's buffers -- it gets a prefix of the mesh.
 *   - workspace: device memory, 16-byte aligned, O(bricks) not O(cells).  With
 *     B_c = ceil(n[c] / 8), B = B_0 B_1 B_2 bricks and C = ceil(B / 1024):
 *     sdf_mesh_workspace_bytes = 88 B + 24 C (per brick a 512-bit activity
 *     mask, two 32-bit counts and two 64-bit offsets; per 1024 bricks three
 *     64-bit sums of the offset scan).  512^3 cells: 23 MB.
 *   - lattice: point (i0, i1, i2), 0 <= i_c <= n[c], lies at p.c = RN(origin[c] +
 *     RN((float)i_c cell[c])); w = RN(f(p) - iso), f bit for bit what sdf_sample
 *     returns for p with this scene, precision and dispatch.  A point is inside
 *     iff w < 0: a NaN or a zero is outside.
 *   - cells: cell (i0, i1, i2), 0 <= i_c < n[c], is active when some corner is
 *     inside and some corner is not.
 *   - edges: edge e = 4a + s + 2t of a cell (s, t in {0, 1}) runs along a from
 *     corner A (offset 0 along a, s along u, t along v) to B (offset 1 along a);
 *     it crosses when inside(A) != inside(B); its parameter is tau = RN(w_A /
 *     RN(w_A - w_B)), its local point q has q_a = tau, q_u = s, q_v = t.
 *   - vertex of an active cell: S_c = the fp32 sum of q_c over the crossing edges
 *     in increasing e, starting at 0; m their number; g_c = RN(S_c / (float)m);
 *     vertex.c = RN(p_c(corner 000) + RN(g_c cell[c])).
 *   - order: cells are grouped into bricks of 8 x 8 x 8, brick (b2 B_1 + b1) B_0 +
 *     b0, local index (l2 8 + l1) 8 + l0; vertices are numbered over the active
 *     cells in increasing (brick, local) order.
 *   - triangles: active cells in that same order; for a = 0, 1, 2 the cell's edge
 *     e = 4a (from corner 000 along a) emits when it crosses and i_u >= 1 and i_v
 *     >= 1: one quad over the four cells that share it, K0 = cell - e_u - e_v, K1
 *     = cell - e_v, K2 = cell, K3 = cell - e_u, reversed to (K3, K2, K1, K0) when
 *     corner 000 is not inside, written as (q0, q1, q2), (q0, q2, q3) in vertex
 *     numbers.  Normals point out of the inside.  Edges on the grid's border
 *     emit nothing: a surface that leaves the grid ends in an open rim.
 *   - normal (optional): what sdf_sample gives at the vertex position
 *     (normal_mode, normal_eps); prim (optional): the owner fold of "Queries"
 *     at the vertex, 0 for a Mandelbulb.
 *   - skipping: a brick whose centre value proves that no lattice point of it
 *     can change sign (|f(centre) - iso| above the scene's Lipschitz constant
 *     times half the brick's diagonal, plus a margin for fp32 rounding:
 *     sdf3d_amd/csrc/mesh_kernel.inc) is not evaluated.  The mesh is bit for bit
 *     the same with and without it; SDF_MESH_DENSE evaluates every brick.  A
 *     Mandelbulb, and a grid or scene beyond the proof's range (coordinates or
 *     parameters above 2^20, n[c] of 2^24 and more), always run dense.
 *   - params: normal_eps, normal_mode, precision and dispatch are used,
 *     validated as sdf_validate_query does.  Dispatch follows the queries': a
 *     built-in variant when the scene matches one, under SDF_DISPATCH_AUTO
 *     run-time specialised mesh kernels for any other primitive list (two,
 *     counted by sdf_jit_count; the generic kernel with SDF3D_JIT=0), GENERIC
 *     and UNCULLED as there.
 *   - SDF_E_INVALID_ARG, decided before any device call (sdf_validate_mesh is
 *     that check of scene, params and grid): everything sdf_validate_query
 *     rejects; grid, workspace or counts NULL; n[c] < 1 or more than 2^30
 *     lattice points; a cell size that is not finite and > 0; origin, iso or the
 *     far corner origin + n cell non-finite or beyond 1e15; unknown flags or a
 *     nonzero reserved; a workspace that is misaligned or smaller than
 *     sdf_mesh_workspace_bytes; emit: out NULL, verts or tris NULL with a
 *     positive capacity, a negative capacity.  Capacities of 0 write nothing.
 *   - asynchronous on `stream`.  SDF_ABI_VERSION stays 12: detect the entry
 *     points by the symbol.
 *   - marching cubes tables, mesh simplification, adaptive grids and several
 *     devices are not offered; sharp edges and corners are "Sharp meshes"
 *     below; vertex colours are sdf_shade_points at the vertices ("Points"). */

/* Sharp meshes (sdf_mesh_emit_sharp: an optional second half of the two-call
 * protocol of "Meshes", after the same sdf_mesh_count on the same workspace.  A
 * surface-nets vertex is the mean of its cell's edge crossings, which chamfers
 * every crease of a hard CSG solid by about a cell; here each crossing is
 * refined along its edge, takes the scene's analytic gradient ("Gradients") as
 * its normal, and the vertex is fitted to those tangent planes inside its cell
 * (dual contouring on the surface-nets topology).  Everything not named below
 * is "Meshes" word for word: lattice, activity, edges, numbering, triangles,
 * prim, the guarded stores, skipping, params and dispatch.  Exact precision
 * rounds every operation once (RN) in the order written and fuses nothing,
 * divisions are IEEE; fast precision may contract and use the hardware
 * reciprocal.  tests/mesh_sharp_ref.py states the block in NumPy:
 *   - identity: sharp NULL, or refine == 0 and iterations == 0, is sdf_mesh_emit
 *     itself, the same kernel and the same bits.  In every case triangles, prim
 *     and the vertex numbering are sdf_mesh_emit's, and normal is what
 *     sdf_sample gives at the vertex written here.
 *   - refinement, per crossing edge (A, B, a, w_A, w_B of "Meshes"): (ta, wa,
 *     tb, wb) = (0, w_A, 1, w_B), tau = RN(w_A / RN(w_A - w_B)); then `refine`
 *     times, always all of them: p = A with p.a = RN(A_a + RN(tau cell[a])); wm =
 *     RN(f(p) - iso), f bit for bit sdf_sample's value; if (wm < 0) == (wa < 0)
 *     then (ta, wa) = (tau, wm), else (tb, wb) = (tau, wm); tau = RN(ta +
 *     RN(RN(tb - ta) RN(wa / RN(wa - wb)))).  One end of the bracket is < 0 and
 *     the other is not, so wa - wb is never 0; a NaN goes where the comparisons
 *     and the arithmetic send it.
 *   - normal of the crossing: n = the gradient of the scene at the final edge
 *     point p (formed from the final tau as above), in exact precision bit for
 *     bit what sdf_sample_grad writes to grad_points for p with upstream NULL;
 *     not normalised.
 *   - mass point: q (q_a = tau, q_u = s, q_v = t), S, m and g_c = RN(S_c /
 *     (float)m) as in "Meshes" with the refined tau.
 *   - fit, over the crossing edges in increasing e, every sum starting at 0:
 *     r_c = RN(RN(q_c - g_c) cell[c]); b = RN(RN(RN(n_0 r_0) + RN(n_1 r_1)) +
 *     RN(n_2 r_2)); A_ij += RN(n_i n_j) for the six i <= j; B_i += RN(n_i b).
 *     tr = RN(RN(A_00 + A_11) + A_22), alpha = RN(1 / tr).  x = 0; `iterations`
 *     times, from the x of the step before: d_i = RN(B_i - RN(RN(RN(A_i0 x_0) +
 *     RN(A_i1 x_1)) + RN(A_i2 x_2))) (A symmetric), then x_i = RN(x_i + RN(alpha
 *     d_i)).  Gradient descent and no SVD: a direction the normals do not
 *     constrain (along a flat face, along an edge) never leaves the mass
 *     point.  If tr is not > 0, or tr or a component of x is not finite, x = 0.
 *   - vertex: l_c = min(max(RN(g_c + RN(x_c / cell[c])), 0), 1) with the GLSL
 *     selects (max(x, y) = x < y ? y : x, min(x, y) = y < x ? y : x); vertex.c =
 *     RN(p_c(corner 000) + RN(l_c cell[c])).  No vertex leaves its cell, so the
 *     mesh keeps the guarantees of surface nets; with x = 0 it is
 *     sdf_mesh_emit's vertex bit for bit.
 *   - dispatch: the lattice, the refinement's f and the signs come from the
 *     variant sdf_mesh_count ran (built-in, run-time specialised -- one more
 *     kernel per signature, counted by sdf_jit_count --, generic, unculled); the
 *     gradient is always the generic fold of "Gradients".
 *   - SDF_E_INVALID_ARG, decided before any device call (sdf_validate_mesh_sharp
 *     is that check of scene, params, grid and sharp): everything sdf_mesh_emit
 *     rejects; refine outside 0 .. 8, iterations outside 0 .. 64, nonzero flags
 *     or reserved.  SDF_E_UNSUPPORTED: a Mandelbulb with a sharp that is neither
 *     NULL nor (0, 0): it has no analytic gradient.  Capacities of 0 write
 *     nothing and launch nothing.
 *   - a full QEF or SVD solve, feature-angle thresholds, vertices outside their
 *     cell, intersection-free guarantees beyond surface nets' and sharp
 *     placement for the Mandelbulb are not offered. */

/* Points (sdf_shade_points: the shading pipeline of "Materials" entered at a
 * point of the caller's own instead of behind a primary march -- vertex colours
 * for an exported mesh, lightmap texels, irradiance probes, a per-vertex
 * occlusion term).  Entry i of every output belongs to point i.  The blocks
 * above are reused word for word, so exact precision can be checked bit for bit
 * (tests/points_ref.c states it over the CPU oracle).  Exact precision rounds
 * every operation once and fuses nothing; fast precision may contract and uses
 * the hardware reciprocal square root, as everywhere else:
 *   - normal: Q = points[i].  With `normals` NULL, N is what sdf_sample returns
 *     as the normal at Q (normal_mode, normal_eps); otherwise N = normals[i]
 *     unchanged, unit or not.
 *   - lift: P = Q when lift == 0 (the bits of Q); otherwise P.c = RN(Q.c + RN(N.c
 *     lift)).  N is not evaluated again at P.  A surface-nets vertex lies up to
 *     half a cell diagonal off the surface, often inside it, and a shadow march
 *     that starts inside the solid means nothing: lift it out first.
 *   - `ao` is the render's occlusion term at (P, N) when SDF_FLAG_AO is set and
 *     ao_taps > 0, else 1.
 *   - `material` is the "Materials" fold at P, all 9 components (amb, dif, ref);
 *     for a Mandelbulb materials[0]'s.
 *   - light i: incident = normalize(L_i - P).  sh_i is the render's shadow march
 *     from o = P + N shadow_offset eps along incident when SDF_FLAG_SHADOW is
 *     set, and its iteration count goes to `steps`; else sh_i = 1 and the count
 *     is 0.  dif_i = clamp(N . incident, 0, 1) sh_i.  With SDF_POINTS_EYE: view =
 *     normalize(eye - P), x_i = max(N . normalize(incident + view), 0), and
 *     spec_i is the precision's own pow of "Lights".  Without the flag no view
 *     is formed and spec_i = +0 enters the sum as a value.  `shadow` and `steps`
 *     hold entry i * nlights + light.  With `shadow` or `steps` asked for, every
 *     shadow march runs to the reference's break, as a render's with step
 *     counts does; `rgba` has the same bits either way.
 *   - `rgba` is the "Lights" / "Materials" colour sum with the point's blended
 *     components, alpha 1.  The buffer must be 16-byte aligned (a point's colour
 *     is stored as one word); the other outputs need their elements' 4 bytes.
 *   - identity with the render: in exact precision, with `normals` NULL, lift 0
 *     and eye = O_0, and with P_0 = O_0 + D_0 d formed as the render forms it,
 *     `rgba` is sdf_render_materials's pixel bit for bit, `steps` for one light
 *     its steps[..][1], and `ao` and dif channels 0 and 1 of SDF_FORMAT_SHADE32F.
 *   - outputs not asked for cost nothing, each decision a uniform branch: no
 *     light loop without rgba, shadow and steps; no fold without rgba and
 *     material; no occlusion taps without rgba and ao.
 *   - params: the march, shadow, normal, AO, precision and dispatch fields are
 *     used.  width, height, samples and output_format are ignored: a copy with
 *     those at sdf_defaults' values is what is validated, with a default camera.
 *   - dispatch follows the queries': a built-in variant when the scene matches
 *     one, under SDF_DISPATCH_AUTO a run-time specialised points kernel for any
 *     other primitive list (counted by sdf_jit_count; the generic kernel with
 *     SDF3D_JIT=0), GENERIC and UNCULLED as there.
 *   - SDF_E_INVALID_ARG, decided before any device call (sdf_validate_points is
 *     that check without the outputs): pts or out NULL; every output NULL; an
 *     rgba that is not 16-byte aligned; NULL
 *     points with n > 0; n < 0 or n > 2^30; unknown flag bits or a nonzero
 *     reserved; a lift that is not finite, negative or above 1e15; with
 *     SDF_POINTS_EYE an eye component that is not finite or above 1e15 in
 *     magnitude; anything sdf_validate_materials rejects with a default camera
 *     (its SDF_E_UNSUPPORTED cases, such as differing shininess, stay
 *     SDF_E_UNSUPPORTED).  n = 0 is SDF_OK: nothing is launched, no buffer is
 *     touched and no device is needed.
 *   - device data: points must be finite and at most 1e15 in magnitude, the
 *     caller's duty as under "Queries"; supplied normals are used as the
 *     arithmetic says.  No address or loop bound depends on either.
 *   - a wave shades 64 consecutive points: order them in coherent groups.
 *   - asynchronous on `stream`.  SDF_ABI_VERSION stays 12: detect the entry
 *     points by the symbol.
 *   - reflections and an environment at points, per-point eyes, output formats
 *     other than fp32 and several devices are not offered. */

/* Gradients (sdf_sample_grad: how the scene function f changes with the points
 * and with the scene's own parameters -- fitting primitives to a point cloud,
 * recovering a scene from depths, optimising a CSG design; sdf3d_amd/autograd.py
 * puts torch.autograd on top).  Primitive scenes only.  With g_i = upstream[i]
 * (1 when upstream is NULL):
 *   - dist[i] = f(points[i]): in exact precision bit for bit what sdf_sample
 *     writes (the same evaluators run).
 *   - grad_points[i] = g_i grad_p f(p_i): the analytic gradient of the scene
 *     spec, not the finite-difference normal, and not normalised.
 *   - grad_prims is float[SDF_MAX_PRIMS][16], the sixteen 4-byte slots of
 *     sdf_primitive: slot 2 = sum_i g_i df/dk, slot 4 + j = sum_i g_i df/dp[j], with
 *     respect to the PUBLIC fields (a round box's half extents and r, a capsule's
 *     end points a and b, the blend radius k).  Slots 0, 1 and 3 (kind, op,
 *     reserved), every parameter slot the kind does not use, the k of a hard
 *     operator and every primitive >= scene->count are written as 0: all 256
 *     floats are written by every call with n > 0.
 *   - the derivative is that of the scene spec's operation sequence, as
 *     reverse-mode differentiation gives it.  A select (min, max, clamp, abs)
 *     passes the adjoint to the operand the forward comparison took (min(x, y) =
 *     y < x ? y : x, max(x, y) = x < y ? y : x, |x|' = -1 for x < 0, else 1); on an
 *     exact tie either one-sided derivative may come out.  A square root's
 *     derivative uses a guarded reciprocal, 1 / len for len > 0 and 0 otherwise
 *     (inside a box, on a torus' or cylinder's axis, at a sphere's centre), so
 *     finite points, a finite upstream and a validated scene give finite outputs.
 *   - the fold: with (a, b) the pair "Materials" defines for primitive i's
 *     operator and m the min or smooth-min, the running value is m(d, v) for the
 *     unions, -m(-d, v) for the subtractions, -m(-d, -v) for the intersections.
 *     Hard: m_a = (b < a) ? 0 : 1, m_b = 1 - m_a, m_k = 0.  Smooth, with the
 *     smooth-min's h as the material fold forms it in the request's precision:
 *     m_a = (b < a) ? h/2 : 1 - h/2, m_b = 1 - m_a, m_k = h h / 4 - h / 2.  d = +-INF
 *     before primitive 0 gives h = 0 and no NaN.
 *   - precision: exact rounds every operation once, fuses nothing and divides
 *     and takes square roots as IEEE does; fast may contract and uses the
 *     hardware reciprocal, reciprocal square root and square root.
 *   - grad_prims is deterministic: no floating-point atomics; the lanes' terms
 *     are summed across each wave, the waves' sums per workgroup in fp64, and
 *     the workgroups' rows (fp32, in `workspace`) in index order in fp64, rounded
 *     once.  The order depends on n only: equal inputs give equal bits.
 *   - workspace: device memory, 16-byte aligned, sdf_grad_workspace_bytes(n) =
 *     1024 min(ceil(n / 256), 1024) bytes (at most 1 MiB: the launch is
 *     grid-stride over a capped grid); needed only with grad_prims.
 *   - dispatch: always the generic kernel evaluating every primitive (an
 *     optimisation loop changes the parameters every call, and the backward pass
 *     needs every primitive's value); params->dispatch is validated and
 *     otherwise ignored, nothing is compiled at run time and sdf_jit_count does
 *     not move.  params are used as sdf_sample uses them.
 *   - SDF_E_INVALID_ARG, decided before any device call (sdf_validate_grad is
 *     that check of scene and params): everything sdf_validate_query rejects;
 *     out NULL or all three of its pointers NULL; NULL points with n > 0; n < 0 or
 *     n > 2^30; grad_prims with a NULL, misaligned or undersized workspace (n > 0).
 *     SDF_E_UNSUPPORTED: a Mandelbulb scene.  n = 0 is SDF_OK: nothing is
 *     launched, no buffer is touched and no device is needed.
 *   - device data: points as under "Queries"; no address or loop bound depends
 *     on them.  Asynchronous on `stream`.  SDF_ABI_VERSION stays 12: detect the
 *     entry points by the symbol.
 *   - second derivatives, gradients of shaded colours, gradients through the
 *     Mandelbulb, per-point (unreduced) parameter gradients and several devices
 *     are not offered. */

/* Measures (sdf_measure: how much solid the scene holds inside a regular grid,
 * where its centre of mass lies, what its inertia is and what box it occupies
 * -- the questions behind export, printing, collision and optimising a CSG
 * design; the box also places the grid of a mesh).  The grid is the sdf_grid of
 * "Meshes"; the solid is f(p) < iso.  Every output is an exact sum (or a minimum
 * or maximum) of integer sample indices, so it does not depend on the order of
 * summation, and exact precision can be checked bit for bit
 * (tests/measure_ref.py states it in NumPy over the CPU oracle):
 *   - samples: one per cell of the grid, at the cell's centre.  Sample (i0, i1,
 *     i2), 0 <= i_c < n[c], lies at p.c = RN(origin[c] + RN(((float)i_c + 0.5f)
 *     cell[c])); the sum (float)i_c + 0.5f is exact.  w = RN(f(p) - iso), f bit for
 *     bit what sdf_sample returns for p with this scene, precision and dispatch.
 *     A sample is inside iff w < 0: a NaN or a zero is outside, as in "Meshes".
 *   - a row is SDF_MEASURE_SLOTS = 16 int64 over a set of inside samples:
 *       slot 0        N, the number of samples                     (empty set: 0)
 *       slots 1..3    S_c = the sum of i_c                                     (0)
 *       slots 4..9    Q = the sums of i0 i0, i1 i1, i2 i2, i0 i1, i0 i2, i1 i2  (0)
 *       slots 10..12  lo_c = the smallest i_c                               (n[c])
 *       slots 13..15  hi_c = the largest i_c                                  (-1)
 *   - rows: row 0 covers all inside samples.  With SDF_MEASURE_OWNERS, row 1 + k
 *     (k = 0 .. SDF_MAX_PRIMS - 1) covers the inside samples whose owner is
 *     primitive k: the owner fold of "Queries" at p, 0 for a Mandelbulb.  Rows of
 *     primitives >= scene->count are empty rows.  With the flag `moments` holds
 *     all SDF_MEASURE_ROWS = 17 rows, without it row 0 alone; every slot of every
 *     row is written by every call.  A scene with a ground plane fills the grid
 *     below the plane: the owner rows are how a caller leaves the plane out, and
 *     how a density per primitive becomes a mass.
 *   - counts (device, 4 int64): [0] bricks whose samples were evaluated, [1]
 *     bricks taken in closed form (proven inside throughout), [2] bricks in all,
 *     [3] 0.
 *   - skipping: bricks are those of "Meshes", 8 x 8 x 8 cells in the same
 *     numbering, and the test is the mesh's, at the mesh's centre point (lattice
 *     point 8 b + 4) against the same bound: the proof (sdf3d_amd/csrc/
 *     mesh_kernel.inc) covers the cell centres of the brick too
 *     (measure_kernel.inc).  A brick proven outside contributes nothing.  A brick
 *     proven inside contributes, without SDF_MEASURE_OWNERS, the closed-form sums
 *     over its index box inside the grid; with the flag it is evaluated, because
 *     owners vary inside it.  The result is bit for bit the same with and without
 *     skipping; SDF_MESH_DENSE in grid->flags evaluates every brick.  A
 *     Mandelbulb, and a grid or scene beyond the proof's range, always run dense,
 *     as "Meshes" says.
 *   - limits: n[c] <= 65536 per axis on top of sdf_validate_mesh's checks; with
 *     at most 2^30 cells every slot and every partial sum stays below 2^62.
 *   - workspace: device memory, 16-byte aligned; with B bricks and R = 17 rows
 *     with SDF_MEASURE_OWNERS, else 1: sdf_measure_workspace_bytes = 8 min(B, 4096)
 *     (16 R + 4) (the launch is grid-stride over a capped number of workgroups, and
 *     each writes its rows once; a second kernel combines them -- no atomics, no
 *     initialisation).  It needs no initialisation and its contents after the
 *     call are unspecified.
 *   - params and dispatch: as "Meshes" (under SDF_DISPATCH_AUTO one run-time
 *     specialised kernel per signature, precision and flag, a family of its own
 *     counted by sdf_jit_count; GENERIC and UNCULLED as there).
 *   - SDF_E_INVALID_ARG, decided before any device call (sdf_validate_measure is
 *     that check of scene, params, grid and flags): everything sdf_validate_mesh
 *     rejects; n[c] > 65536; unknown flag bits; moments or counts NULL; a
 *     workspace that is NULL, not 16-byte aligned or smaller than
 *     sdf_measure_workspace_bytes.
 *   - host conversion, in fp64 over the real-valued lattice coordinates origin +
 *     (i + 1/2) cell (not over the rounded fp32 sample positions), with c_c =
 *     cell[c], for a row with N > 0:
 *       volume      = N c0 c1 c2
 *       centroid_c  = origin_c + (S_c / N + 1/2) c_c
 *       covariance  C_cd = (Q_cd / N - (S_c / N)(S_d / N)) c_c c_d + [c = d] c_c^2 / 12
 *       inertia about the centroid = mass (tr(C) Id - C)
 *       bounds      = [origin + lo c, origin + (hi + 1) c]
 *     With a density rho_k per primitive the raw moments of the owner rows are
 *     combined first, sum_k rho_k (N_k, S_k, Q_k), and the same formulas follow
 *     (mass = sum_k rho_k N_k c0 c1 c2).
 *   - asynchronous on `stream`.  No loop bound and no address depends on a
 *     sampled value.  SDF_ABI_VERSION stays 12: detect the entry point by the
 *     symbol.
 *   - surface area (sum the mesh's triangles), partial-cell occupancy or sub-cell
 *     sampling (pass a finer grid), several devices and gradients of the
 *     measures are not offered. */

/* Framebuffer element formats (4 channels R,G,B,A per pixel).
 *   RGBA32F  the shader's float fragment_color (voxel_fragment.frag:12,210).
 *   RGBA16F  IEEE half, round to nearest even.
 *   RGBA8    what the reference's RGBA8 window shows (main.cpp:95-96):
 *            u8 = trunc(min(max(c, 0), 1) * 255 + 0.5), NaN -> 0, no
 *            multiply-add fusion.
 *   RGB32F   RGBA32F without the alpha channel, which the shader always
 *            writes as 1.0 (voxel_fragment.frag:210): a lossless 12-byte
 *            wire format for multi-device frames; sdf_deinterleave expands
 *            it to an RGBA32F frame with alpha = 1.
 *   SHADE32F the pixel's three shading terms instead of its colour, as
 *            RGBA32F (ao, dif, x, 1): ao the AO factor (1 without AO), dif =
 *            clamp(N.L, 0, 1) * shadow, x = max(N.H, 0); the colour is
 *            la * amb * ao + dif * mat.dif + pow(x, shininess) * mat.ref
 *            (voxel_fragment.frag:204-210) in the precision's fixed operation
 *            sequence (sdf3d_amd/csrc/shade.h).  Diagnostics: what TILES
 *            streams carry.
 *   TILES    the frame losslessly compressed for the multi-device gather
 *            (about 2.3 instead of 12 bytes per pixel on the 4K CSG scene),
 *            decoded bit for bit by sdf_tiles_decode.  A rendered stream
 *            carries the SHADE32F terms in its three channels (smoother than
 *            the colour, which mixes them: 29 % fewer bytes) and the frame's
 *            shading constants in its header; the decoder makes the colour
 *            from them exactly as sdf_render does.  The rendered (packed) rows
 *            are cut into 8x8 tiles, tile t = ty * ceil(width / 8) + tx
 *            covering packed rows 8ty.. and columns 8tx..; pixel j = 8 *
 *            row + column of a tile.  Per tile and channel: the float bits
 *            mapped to ordered integers u (bits ^ 0x7fffffff when the sign
 *            is set, an involution; u = 0 outside the frame), the gradient
 *            residual u - left - up + upleft (neighbours outside the tile
 *            are 0; mod 2^32; its inverse is the tile's 2-D prefix sum),
 *            zigzag-coded to z, with z := 0 for pixel 0 (it travels raw) and
 *            for pixels outside the frame.  Per channel c the tile stores
 *            the low b[c] bits of every z_j, pixel by pixel: b[c] u64 words
 *            whose bits j b[c] .. j b[c] + b[c] - 1 are z_j's (ABI 10; bit
 *            planes before), and, when its widest z has w > b[c] bits, an
 *            escape: a u64 mask of the outlier pixels (z_j >= 2^b[c]), a
 *            width byte d = w - b[c]
 *            and each outlier's bits b[c].. as a d-bit field.  The encoder
 *            picks b[c] among w, w - 1, .., w - 12 by the smallest size
 *            (64 b + 72 + d * outliers bits; ties: larger b).
 *            Stream layout (little-endian; sdf_tiles_bytes() sizes the
 *            buffer, stream plus the encoder's scratch):
 *              u32 used             bytes of tile data
 *              u32 ntiles
 *              u32 shade            0: the channels are RGB (a stream not
 *                                   made by sdf_render); 1 / 2: shading
 *                                   terms of a fast / exact render
 *              u32 0
 *              f32 lam[3]           light.ambient * material.amb[c] (fp32)
 *              f32 dif[3], ref[3]   material.dif, material.ref
 *              f32 shininess
 *              u32 0, 0
 *              u32 offset[ntiles]   (at byte 64) tile t's data at data +
 *                                   offset[t]
 *              head = stream + align16(64 + 4 * ntiles):
 *                u32x4 head[ntiles] {b0 | b1 << 6 | b2 << 12 | q << 18 |
 *                                   e << 26, first[3]}: q the tile's data
 *                                   in u64 words, e bit c set when channel
 *                                   c is escaped (P = popcount(e)),
 *                                   first[c] u of pixel 0
 *              data = head + 16 * ntiles, per tile q u64 words:
 *                                   b0 + b1 + b2 words of base bits,
 *                                   channel by channel; the P masks of the escaped
 *                                   channels; then one bitstream (LSB
 *                                   first, zero-padded to whole words):
 *                                   the P width bytes, then the fields
 *                                   pixel by pixel, each pixel's fields of
 *                                   the channels it is an outlier of in
 *                                   channel order
 *            The meaningful prefix of a stream is data + used bytes; tile
 *            blocks appear in tile order (tests/tiles_ref.py states the
 *            codec in NumPy).                                             */
typedef enum {
  SDF_FORMAT_RGBA32F = 0,
  SDF_FORMAT_RGBA16F = 1,
  SDF_FORMAT_RGBA8 = 2,
  SDF_FORMAT_RGB32F = 3,
  SDF_FORMAT_TILES = 4,
  SDF_FORMAT_SHADE32F = 5
} sdf_format;

typedef enum {
  SDF_DISPATCH_AUTO = 0,       /* specialised kernel: a built-in one when the
                                  scene matches, else one compiled at run time
                                  for the scene's (kind, op) sequence (hipRTC,
                                  ~0.7 s once per sequence and process; off
                                  with SDF3D_JIT=0), else the generic kernel  */
  SDF_DISPATCH_GENERIC = 1,    /* always the generic primitive-list kernel     */
  SDF_DISPATCH_UNCULLED = 2    /* generic kernel evaluating every primitive at
                                  every point (no bounding-volume culling): the
                                  straight restatement, for cross-checks       */
} sdf_dispatch;

/* Which rows of the frame a call renders.  Rows are grouped into blocks of
 * `block_rows` rows; block b (rows [b*block_rows, (b+1)*block_rows)) is
 * rendered iff b >= first_block and, with o = (b - first_block) %
 * block_stride, o % step == 0 and o / step < run: run = max(block_run, 1)
 * blocks per period of `block_stride` blocks, step = max(run_step, 1) blocks
 * apart (step 1: consecutive).  Rendered rows are written densely ("packed")
 * in increasing y order, so {block_rows = 8, first_block = r, block_stride =
 * N} is device r's share of an N-device interleaved tiling and {8, 0, 1} is
 * the whole frame; runs give devices unequal shares (the multi-device frame
 * driver gives rank 0, which also assembles the frame, fewer rows:
 * {8, 0, P, 0, a, 1} for it and {8, a + r - 1, P, 0, b, N - 1} for rank
 * r >= 1, P = a + b (N - 1): the peers' blocks interleave inside the period,
 * so a frame whose block count is not a multiple of P gives its last partial
 * period's blocks to distinct ranks).                                        */
typedef struct {
  int32_t block_rows;
  int32_t first_block;
  int32_t block_stride;
  int32_t flags;      /* sdf_tiling_flags (0: packed rows) */
  int32_t block_run;  /* blocks per period (0 or 1: one) */
  int32_t run_step;   /* blocks between a run's blocks (0 or 1: consecutive);
                         (run - 1) * step < block_stride */
} sdf_tiling;

/* SDF_TILING_FRAME_ROWS: write the owned rows at their frame positions (the
 * buffer holds `height` rows, the others untouched) instead of packed --
 * rank 0 of a multi-device frame renders its share straight into the
 * assembled frame.  Not with SDF_FORMAT_TILES. */
typedef enum { SDF_TILING_FRAME_ROWS = 1 } sdf_tiling_flags;

/* ---- entry points -------------------------------------------------------- */

/* The packed tiling of `rank`'s share of a `world`-device frame: rank 0
 * share_root consecutive blocks and every other rank share_peer blocks,
 * world - 1 apart, per period of share_root + share_peer * (world - 1)
 * 8-row blocks (1:1 = plain interleave; world 1 = the whole frame). */
int sdf_share_tiling(int32_t rank, int32_t world, int32_t share_root, int32_t share_peer,
                     sdf_tiling* tiling);

/* ABI version of the loaded library (== SDF_ABI_VERSION when compatible). */
int sdf_abi_version(void);

/* Fill every non-null struct with the reference defaults (see top comment).
 * `width`/`height` set params->width/height (<= 0: 800 x 600, main.cpp:4-5). */
int sdf_defaults(sdf_scene* scene, sdf_camera* camera, sdf_light* light,
                 sdf_material* material, sdf_params* params,
                 int32_t width, int32_t height);

/* Validate a request without touching the device. */
int sdf_validate(const sdf_scene* scene, const sdf_camera* camera,
                 const sdf_light* light, const sdf_material* material,
                 const sdf_params* params, const sdf_tiling* tiling);

/* Number of rows a tiling owns in a frame of `height` rows (>= 0), or a
 * negative SDF_E* code. */
int sdf_owned_rows(int32_t height, const sdf_tiling* tiling);

/* Bytes per pixel of a sdf_format (16, 8, 4, 12, -, 16), or a negative SDF_E* code
 * (SDF_E_UNSUPPORTED for TILES, whose size is per stream). */
int sdf_format_bytes(int32_t format);

/* Capacity in bytes of a TILES stream of `rows` packed rows of `width`
 * pixels (the worst case: 32-bit residuals), or a negative SDF_E* code
 * (SDF_E_UNSUPPORTED when that worst case would not fit the stream's 32-bit
 * offsets: more than ~5.6M tiles, ~358 Mpixels; sdf_render refuses such a
 * TILES render the same way). */
int64_t sdf_tiles_bytes(int32_t width, int32_t rows);

/* Render the rows owned by `tiling` (NULL = whole frame) into `rgba`
 * (device, owned_rows * width pixels of params->output_format, packed as
 * described above).
 * `steps` (device, may be NULL) receives 2 int32 per pixel: the primary and
 * the shadow march iteration counts (diagnostics / flop accounting).
 * With params->samples > 1 every output pixel is the resolve of its S x S
 * sub-samples and `steps` holds the sub-samples' counts ("Supersampling"
 * above).  Asynchronous on `stream`. */
int sdf_render(const sdf_scene* scene, const sdf_camera* camera,
               const sdf_light* light, const sdf_material* material,
               const sdf_params* params, const sdf_tiling* tiling,
               void* rgba, int32_t* steps, void* stream);

/* Render schedules.  A frame's cost is uneven: grazing rays near the horizon
 * march long, so a launch whose last waves hold the costliest tiles ends
 * with most of the GPU idle.  sdf_render_scheduled is sdf_render dispatching
 * the rows' 8-row blocks in the order a schedule keeps: the kernel adds
 * every wave's shader-clock cycles to its block's counter, the schedule
 * reads the counters back every `period` launches without waiting (pinned
 * copy behind the launch, event polled at the next call), and later launches
 * take the blocks costliest first.  Any order renders every block exactly
 * once: the output is bit-identical to sdf_render's.  A schedule serves
 * renders of `rows` packed rows (owned rows of the tiling, <= 4096; others
 * render in launch order) and is not thread-safe; one schedule per stream
 * keeps each stream's measurements its own.  Create / destroy synchronise
 * the device. */
typedef struct sdf_schedule sdf_schedule;
int sdf_schedule_create(int32_t rows, int32_t period, sdf_schedule** schedule);
int sdf_schedule_destroy(sdf_schedule* schedule);
/* The schedule's current order (blockIdx.y -> 8-row block) into order[0..n):
 * returns the number of blocks it orders, 0 before its first cost snapshot
 * has landed (launch order). */
int sdf_schedule_order(const sdf_schedule* schedule, int32_t* order, int32_t n);
int sdf_render_scheduled(const sdf_scene* scene, const sdf_camera* camera,
                         const sdf_light* light, const sdf_material* material,
                         const sdf_params* params, const sdf_tiling* tiling,
                         void* rgba, int32_t* steps, sdf_schedule* schedule, void* stream);

/* sdf_render / sdf_render_scheduled (`schedule` may be NULL) under `nlights`
 * lights ("Lights" above): the surface is traced once and every light adds
 * its diffuse and specular terms.  sdf_validate_lights is the host-only check
 * sdf_render_lights makes first (no device call). */
int sdf_validate_lights(const sdf_scene* scene, const sdf_camera* camera,
                        const sdf_light* lights, int32_t nlights, int32_t light_flags,
                        const sdf_material* material, const sdf_params* params,
                        const sdf_tiling* tiling);
int sdf_render_lights(const sdf_scene* scene, const sdf_camera* camera,
                      const sdf_light* lights, int32_t nlights, int32_t light_flags,
                      const sdf_material* material, const sdf_params* params,
                      const sdf_tiling* tiling, void* rgba, int32_t* steps,
                      sdf_schedule* schedule, void* stream);

/* sdf_validate_lights / sdf_render_lights with a material per primitive
 * ("Materials" above) in place of the one material.  Additions like the
 * lights entry points: SDF_ABI_VERSION stays 12, detect them by the symbol. */
int sdf_validate_materials(const sdf_scene* scene, const sdf_camera* camera,
                           const sdf_light* lights, int32_t nlights, int32_t light_flags,
                           const sdf_material* materials, int32_t nmaterials,
                           const sdf_params* params, const sdf_tiling* tiling);
int sdf_render_materials(const sdf_scene* scene, const sdf_camera* camera,
                         const sdf_light* lights, int32_t nlights, int32_t light_flags,
                         const sdf_material* materials, int32_t nmaterials,
                         const sdf_params* params, const sdf_tiling* tiling, void* rgba,
                         int32_t* steps, sdf_schedule* schedule, void* stream);

/* sdf_validate_materials / sdf_render_materials with mirror reflections
 * ("Reflections" above).  Additions: SDF_ABI_VERSION stays 12, detect them by
 * the symbol. */
int sdf_validate_reflect(const sdf_scene* scene, const sdf_camera* camera,
                         const sdf_light* lights, int32_t nlights, int32_t light_flags,
                         const sdf_material* materials, int32_t nmaterials,
                         const sdf_reflect* reflect, const sdf_params* params,
                         const sdf_tiling* tiling);
int sdf_render_reflect(const sdf_scene* scene, const sdf_camera* camera,
                       const sdf_light* lights, int32_t nlights, int32_t light_flags,
                       const sdf_material* materials, int32_t nmaterials,
                       const sdf_reflect* reflect, const sdf_params* params,
                       const sdf_tiling* tiling, void* rgba, int32_t* steps,
                       sdf_schedule* schedule, void* stream);

/* sdf_validate_reflect / sdf_render_reflect with an environment ("Environment"
 * above; env NULL: sdf_render_reflect).  Additions: SDF_ABI_VERSION stays 12,
 * detect them by the symbol. */
int sdf_validate_env(const sdf_scene* scene, const sdf_camera* camera,
                     const sdf_light* lights, int32_t nlights, int32_t light_flags,
                     const sdf_material* materials, int32_t nmaterials,
                     const sdf_reflect* reflect, const sdf_environment* env,
                     const sdf_params* params, const sdf_tiling* tiling);
int sdf_render_env(const sdf_scene* scene, const sdf_camera* camera,
                   const sdf_light* lights, int32_t nlights, int32_t light_flags,
                   const sdf_material* materials, int32_t nmaterials,
                   const sdf_reflect* reflect, const sdf_environment* env,
                   const sdf_params* params, const sdf_tiling* tiling, void* rgba,
                   int32_t* steps, sdf_schedule* schedule, void* stream);

/* Ray and point queries ("Queries" above).  Additions: SDF_ABI_VERSION stays
 * 12, detect them by the symbol.  sdf_validate_query is the host-only check
 * the three make first (no device call). */
int sdf_validate_query(const sdf_scene* scene, const sdf_params* params);
int sdf_trace(const sdf_scene* scene, const sdf_params* params, const float* origins,
              const float* dirs, int64_t n, const sdf_hits* hits, void* stream);
int sdf_trace_camera(const sdf_scene* scene, const sdf_camera* camera, const sdf_params* params,
                     const sdf_hits* hits, void* stream);
int sdf_sample(const sdf_scene* scene, const sdf_params* params, const float* points, int64_t n,
               float* dist, float* normal, void* stream);

/* Shading of caller-supplied rays ("Rays" above).  reflect NULL: no bounce;
 * env NULL: no environment.  Additions: SDF_ABI_VERSION stays 12, detect them
 * by the symbol.  sdf_validate_rays is the host-only check sdf_render_rays
 * makes first (no device call). */
int sdf_validate_rays(const sdf_scene* scene, const sdf_light* lights, int32_t nlights,
                      int32_t light_flags, const sdf_material* materials, int32_t nmaterials,
                      const sdf_reflect* reflect, const sdf_environment* env,
                      const sdf_params* params, const sdf_rays* rays);
int sdf_render_rays(const sdf_scene* scene, const sdf_light* lights, int32_t nlights,
                    int32_t light_flags, const sdf_material* materials, int32_t nmaterials,
                    const sdf_reflect* reflect, const sdf_environment* env,
                    const sdf_params* params, const sdf_rays* rays, void* rgba, int32_t* steps,
                    void* stream);
int sdf_camera_rays(const sdf_camera* camera, const sdf_params* params, float* origins,
                    float* dirs, void* stream);

/* Shading at caller-supplied points ("Points" above).  Additions:
 * SDF_ABI_VERSION stays 12, detect them by the symbol.  sdf_validate_points is
 * the host-only check sdf_shade_points makes first (no device call). */
int sdf_validate_points(const sdf_scene* scene, const sdf_light* lights, int32_t nlights,
                        int32_t light_flags, const sdf_material* materials, int32_t nmaterials,
                        const sdf_params* params, const sdf_points* pts);
int sdf_shade_points(const sdf_scene* scene, const sdf_light* lights, int32_t nlights,
                     int32_t light_flags, const sdf_material* materials, int32_t nmaterials,
                     const sdf_params* params, const sdf_points* pts,
                     const sdf_point_shade* out, void* stream);

/* Isosurface meshes ("Meshes" above).  Additions: SDF_ABI_VERSION stays 12,
 * detect them by the symbol.  sdf_validate_mesh is the host-only check both
 * calls make first (no device call); sdf_mesh_workspace_bytes the size of the
 * workspace of `grid`, or a negative SDF_E* code. */
int sdf_validate_mesh(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid);
int64_t sdf_mesh_workspace_bytes(const sdf_grid* grid);
int sdf_mesh_count(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                   void* workspace, int64_t workspace_bytes, int64_t* counts /* device, 4 */,
                   void* stream);
int sdf_mesh_emit(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                  void* workspace, int64_t workspace_bytes, const sdf_mesh_out* out,
                  void* stream);
/* Sharp-feature vertices ("Sharp meshes" above).  Additions likewise.  `sharp`
 * may be NULL: sdf_mesh_emit. */
int sdf_validate_mesh_sharp(const sdf_scene* scene, const sdf_params* params,
                            const sdf_grid* grid, const sdf_mesh_sharp* sharp);
int sdf_mesh_emit_sharp(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                        const sdf_mesh_sharp* sharp, void* workspace, int64_t workspace_bytes,
                        const sdf_mesh_out* out, void* stream);

/* Gradients ("Gradients" above).  Additions: SDF_ABI_VERSION stays 12, detect
 * them by the symbol.  sdf_validate_grad is the host-only check of scene and
 * params (no device call); sdf_grad_workspace_bytes the size of the workspace for
 * n points (0 for n = 0), or a negative SDF_E* code. */
int sdf_validate_grad(const sdf_scene* scene, const sdf_params* params);
int64_t sdf_grad_workspace_bytes(int64_t n);
int sdf_sample_grad(const sdf_scene* scene, const sdf_params* params, const float* points,
                    int64_t n, const float* upstream /* device, n; NULL: every g_i = 1 */,
                    const sdf_grad_out* out, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* Measures ("Measures" above).  Additions: SDF_ABI_VERSION stays 12, detect
 * them by the symbol.  sdf_validate_measure is the host-only check of scene,
 * params, grid and flags (no device call); sdf_measure_workspace_bytes the size
 * of the workspace of `grid` under `flags`, or a negative SDF_E* code. */
int sdf_validate_measure(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                         int32_t flags);
int64_t sdf_measure_workspace_bytes(const sdf_grid* grid, int32_t flags);
int sdf_measure(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                int32_t flags /* SDF_MEASURE_* */, void* workspace, int64_t workspace_bytes,
                int64_t* moments /* device, rows x 16 */, int64_t* counts /* device, 4 */,
                void* stream);

/* Scatter `nparts` packed row-block buffers (part r = rank r's output for
 * tiling {block_rows, r, nparts}), laid out back to back in `parts` with a
 * pitch of `part_stride_rows` rows each, into the full frame `frame`
 * (height * width pixels of `format`; RGB32F parts produce an RGBA32F frame
 * with alpha = 1).  Device pointers; asynchronous on `stream`. */
int sdf_deinterleave(const void* parts, int32_t nparts,
                     int32_t part_stride_rows, int32_t width, int32_t height,
                     int32_t block_rows, int32_t format, void* frame, void* stream);

/* Decode `nparts` TILES streams (part r = rank r's output for tiling
 * {block_rows, r, nparts}; nparts = 1 with block_rows = height for a whole
 * frame), laid out back to back in `parts` with a pitch of `part_stride`
 * bytes, into the RGBA32F frame `frame` (height * width, alpha = 1): the
 * de-interleave of sdf_deinterleave fused with the decode.  A part whose
 * header says ntiles = 0 is skipped (its rows rendered into the frame by
 * other means, e.g. SDF_TILING_FRAME_ROWS).  Device pointers; asynchronous
 * on `stream`.
 * sdf_tiles_decode_tilings: part r holds the rows of tilings[r] (a host
 * array of nparts packed tilings, at most SDF_MAX_DECODE_PARTS), e.g. the
 * unequal shares of the frame driver; sdf_tiles_decode is the interleaved
 * case tilings[r] = {block_rows, r, nparts, 0, 1}. */
#define SDF_MAX_DECODE_PARTS 64
int sdf_tiles_decode_tilings(const void* parts, int32_t nparts, int64_t part_stride,
                             const sdf_tiling* tilings, int32_t width, int32_t height,
                             void* frame, void* stream);
int sdf_tiles_decode(const void* parts, int32_t nparts, int64_t part_stride,
                     int32_t width, int32_t height, int32_t block_rows, void* frame,
                     void* stream);

/* Streams are untrusted input (they crossed a wire): every decode reads only
 * inside each part's worst-case stream (sdf_tiles_bytes of its rows), and a
 * malformed part -- header length or tile count that disagrees with the
 * part, a tile whose offset, size or base widths leave the stream's data, an
 * escape field beyond its tile -- is skipped (the whole part, or the tiles
 * concerned: nothing is written for them; every other tile decodes as
 * usual).  sdf_tiles_decode(_tilings) skip silently;
 * sdf_tiles_decode_checked reports:
 *   used    host array of nparts (may be NULL): the data bytes part r must
 *           hold (its header word 0, e.g. the length the ranks agreed on
 *           before the transfer), or -1 for "the header's own, within the
 *           part"; a part expected to carry a stream (used[r] >= 0) whose
 *           header says none is malformed;
 *   status  device-writable array of nparts uint32 (may be NULL), zeroed by
 *           the caller: word r becomes nonzero (SDF_TILES_BAD_* bits) when
 *           part r is malformed -- asynchronous, like the decode.  With
 *           status == NULL the call waits for the decode on `stream` and
 *           returns SDF_E_COMM when some part was malformed. */
/* One byte per cause (ABI 11): each is set by a byte store of its own, so
 * the causes of a part combine without atomics (waves of one part race). */
#define SDF_TILES_BAD_HEADER 0x000001u
#define SDF_TILES_BAD_TILE   0x000100u
#define SDF_TILES_BAD_FIELD  0x010000u
int sdf_tiles_decode_checked(const void* parts, int32_t nparts, int64_t part_stride,
                             const sdf_tiling* tilings, const int64_t* used, int32_t width,
                             int32_t height, void* frame, uint32_t* status, void* stream);

/* Debug view of the `steps` output of sdf_render: `count` int2 entries
 * (primary, shadow) -> colours of `format`, with which = 0 (primary), 1
 * (shadow) or 2 (their sum), intensity = steps / max_steps mapped through the
 * Turbo colormap the reference ships unused (Code/kernel/utilities.cl:7-284:
 * its 256-entry table, index round(255 * intensity) rounded half away from
 * zero and clamped to [0, 255], alpha 1).  Device
 * pointers; asynchronous on `stream`. */
int sdf_heatmap(const int32_t* steps, int32_t count, int32_t which, int32_t max_steps,
                int32_t format, void* out, void* stream);

/* Number of scene signatures compiled at run time in this process (see
 * SDF_DISPATCH_AUTO). */
int sdf_jit_count(void);

/* Build identity of the built-in render kernels of `precision`
 * (SDF_PRECISION_*): 16 hex digits of a SHA-256 over the kernel's sources
 * (its translation unit, render_kernel.inc and the layer files it includes,
 * kernel_args.h, wave_bits.h, shade.h, cr_math.h, sdf_abi.h), its compile flags and the compiler's version, fixed when the
 * library is built.  Measurement tools store it beside counters taken from
 * the kernel, so a counter summary is never applied to another build.
 * NULL for an unknown precision. */
const char* sdf_kernel_id(int32_t precision);

/* The culling bounds the generic kernel reads for a primitive scene (host
 * only, no device needed; diagnostics and tests).  A plan of the fixed-scene
 * or run-time specialised kernels (SDF_DISPATCH_AUTO) caches gaps along a
 * path and reads larger ones: 2^-20 (|c|_inf + R_i + k_i + max_dist) is added
 * to the 1e-4 below.  No plan culls when a cullable primitive has |c|_inf +
 * R_i + k_i + max_dist > 2^22; this call knows no max_dist and reports
 * *cluster_first = count from |c|_inf + R_i + k_i > 2^22 on.  Per primitive
 * bounds[4 * i ..] = {centre.xyz, K_i = (k_i + R_i + 1e-4) / (1 - 1e-5)}
 * with R_i the radius of a sphere containing primitive i, the cluster
 * cluster[0..3] = {centre.xyz, K} of the sphere containing primitives
 * [*cluster_first, count) (K with the largest blend radius), and
 * *cluster_first (= count when nothing is culled).  bounds holds
 * 4 * SDF_MAX_PRIMS floats.  SDF_E_UNSUPPORTED for a Mandelbulb scene. */
int sdf_scene_bounds(const sdf_scene* scene, float* bounds, float* cluster,
                     int32_t* cluster_first);

/* ---- multi-device frame driver ----------------------------------------------
 * One process per GPU.  Every rank renders its row blocks of each frame
 * (tiling with shares: rank 0 `share_root` blocks and every other rank
 * `share_peer` blocks per period of share_root + share_peer * (world - 1))
 * as a TILES stream; rank 0 renders its own rows straight into the frame and
 * assembles the rest: an RCCL all-gather of the streams' lengths, RCCL
 * point-to-point transfers of exactly those bytes to rank 0, and
 * sdf_tiles_decode_tilings into the frame -- bit-identical to a one-device
 * render.  Frames rotate over `nbuf` buffer sets, one HIP stream each; frame
 * i is shipped `lag` frames after its render (the host reads its agreed
 * lengths from pinned memory, without stalling the queue when lag >= 2).
 * The RCCL calls go to two communicators, each on a stream of its own (the
 * lengths; the streams), in the same order on every rank.
 *
 * RCCL is loaded at run time from `rccl_path` (the librccl.so this process
 * already uses, e.g. PyTorch's, so one RCCL instance serves both); the
 * caller exchanges each communicator's 128-byte unique id (rank 0 makes it
 * with sdf_comm_unique_id) through its own channel.
 * world == 1 needs no communicator: frames render whole, nothing is shipped. */
#define SDF_COMM_ID_BYTES 128
typedef struct sdf_comm sdf_comm;
typedef struct sdf_driver sdf_driver;

int sdf_comm_unique_id(const char* rccl_path, void* id /* SDF_COMM_ID_BYTES */);
/* Collective over nranks processes (blocks until all have joined, at most
 * timeout_ms, <= 0: 120000; then SDF_E_TIMEOUT); the current HIP device is
 * the communicator's. */
int sdf_comm_create(const char* rccl_path, const void* id, int32_t nranks, int32_t rank,
                    int32_t timeout_ms, sdf_comm** comm);
int sdf_comm_destroy(sdf_comm* comm);

/* SDF_DRIVER_ROOT_AS_PEER: rank 0 ships its rows as a TILES stream to itself
 * like every other rank (probes of one rank's full per-frame cost on one
 * GPU, world == 1 included). */
#define SDF_DRIVER_ROOT_AS_PEER 0x1
typedef struct {
  int32_t rank, world;
  int32_t share_root, share_peer; /* blocks per period (>= 1; 1:1 = plain interleave) */
  int32_t nbuf;                   /* buffer sets, 2 .. 16 (render streams: <= 4)      */
  int32_t lag;                    /* frames from a batch's last render to its gather,
                                     1 .. nbuf - batch                                */
  int32_t flags;                  /* SDF_DRIVER_*                                     */
  int32_t timeout_ms;             /* host waits give up after this (<= 0: 60000)      */
  int32_t batch;                  /* frames per ship (<= 0: 1): one length
                                     all-gather and one send/recv group per `batch`
                                     consecutive frames; nbuf % batch == 0          */
} sdf_driver_config;

/* The frame format is params->output_format (RGBA32F at world > 1: the wire
 * is lossless TILES).  size_comm, data_comm: two distinct communicators
 * over the `world` ranks, used by this driver alone (NULL when world == 1
 * without ROOT_AS_PEER). */
int sdf_driver_create(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* light,
                      const sdf_material* material, const sdf_params* params,
                      const sdf_driver_config* config, sdf_comm* size_comm, sdf_comm* data_comm,
                      sdf_driver** driver);
/* Camera of the frames stepped from now on (the arcball V_mat of main.cpp:93-94). */
int sdf_driver_set_camera(sdf_driver* driver, const sdf_camera* camera);
/* Enqueue the next frame (index returned in *frame_index, may be NULL). */
int sdf_driver_step(sdf_driver* driver, int64_t* frame_index);
/* Ship every rendered frame and wait until all work of this rank is done. */
int sdf_driver_drain(sdf_driver* driver);
/* Rank 0 (or world 1): device pointer of frame `index`'s framebuffer
 * (height * width pixels), one of the last nbuf frames whose buffer set no
 * later frame has taken (after a drain that closed a short batch the next
 * frames may start on other buffer sets): any other index is
 * SDF_E_INVALID_ARG.  With collectives the frame must have been shipped (the
 * last `lag` frames stepped are, after sdf_driver_drain): an index not
 * shipped yet is SDF_E_INVALID_ARG.  A rank-0 decode that finds a peer's
 * stream malformed (sdf_tiles_decode_checked) fails the driver: the next
 * sdf_driver_step or sdf_driver_drain returns SDF_E_COMM. */
int sdf_driver_frame(sdf_driver* driver, int64_t index, void** rgba);
/* Copy frame `index` (as sdf_driver_frame) into the caller's device buffer
 * `dst` of `bytes` (>= the frame's size), asynchronously on `stream` after
 * all work queued for that frame. */
int sdf_driver_read_frame(sdf_driver* driver, int64_t index, void* dst, int64_t bytes,
                          void* stream);
/* Host-time accounting since creation (n >= 3 values): out[0] frames
 * stepped, out[1] seconds spent inside sdf_driver_step / sdf_driver_drain,
 * out[2] the part of out[1] spent waiting for the GPU or a peer; then the
 * seconds spent enqueueing out[3] renders, out[4] length all-gathers (with
 * their copies and events), out[5] RCCL send/recv groups, out[6] decodes. */
int sdf_driver_stats(sdf_driver* driver, double* out, int32_t n);
int sdf_driver_destroy(sdf_driver* driver);

/* ---- single-process multi-device frames -------------------------------------
 * One frame rendered across `ndev` devices of THIS process (the reference's
 * host is one process, main.cpp:34-110): devices[0] is the root and holds
 * `rgba` (width * height RGBA32F pixels, params->output_format must be
 * SDF_FORMAT_RGBA32F); `stream` is a stream of the root device.  Rows are
 * shared as by the driver (sdf_share_tiling with share_root : share_peer
 * blocks, <= 0: the measured defaults): the root renders its rows into
 * `rgba`, every other device its rows as a TILES stream into a buffer of its
 * own, and the root decodes those streams in place through peer-mapped
 * memory (hipDeviceEnablePeerAccess).  Asynchronous: the frame is complete
 * for work enqueued on `stream` after the call.  Successive calls must be
 * ordered (the same `stream`): they share the library's buffers for this
 * device list, two sets alternating so the peers render the next frame while
 * the root decodes this one.  A device may be listed more than once (its
 * shares then render on it in turn).  The current device is left unchanged. */
int sdf_render_multi(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* light,
                     const sdf_material* material, const sdf_params* params, int32_t ndev,
                     const int32_t* devices, int32_t share_root, int32_t share_peer, void* rgba,
                     void* stream);
/* Wait for and free the buffers sdf_render_multi keeps. */
int sdf_render_multi_release(void);

/* ---- frame sequences ----------------------------------------------------------
 * n whole frames of one scene: frame i seen through cameras[i], written to
 * rgba[i] (width * height pixels of params->output_format; TILES is
 * SDF_E_UNSUPPORTED) and, when `steps` is non-null and steps[i] is, its
 * iteration counts to steps[i] (width * height int2).  Equal bit for bit to
 * n sdf_render calls with the same arguments.  This is the reference's frame
 * loop (main.cpp:87-98) for a camera path known in advance: the frames are
 * rendered by a persistent kernel, up to 16 frames per launch, whose waves
 * take 8x8 tiles of all its frames from one work counter, so a frame's
 * slowest tiles overlap the next frame's first ones.  Asynchronous on
 * `stream` (a stream of the current device).  Every camera is validated
 * before anything is enqueued. */
int sdf_render_frames(const sdf_scene* scene, const sdf_camera* cameras, int32_t n,
                      const sdf_light* light, const sdf_material* material,
                      const sdf_params* params, void* const* rgba, int32_t* const* steps,
                      void* stream);

/* Short description of a status code. */
const char* sdf_strerror(int code);

#ifdef __cplusplus
}
#endif

#endif /* SDF_ABI_H */
