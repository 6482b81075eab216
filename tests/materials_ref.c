/*
 * materials_ref.c -- TEST INFRASTRUCTURE ONLY: the reference of the material
 * fold (include/sdf_abi.h "Materials", sdf_render_materials) over the CPU
 * oracle.  It includes the oracle's translation unit, the way
 * tools/terms_probe.c does, and uses its instrumentation hooks: the pixel
 * hook captures the oracle's own hit point P inside shade_pixel, where the
 * fold is evaluated in plain C over the oracle's f32_sd_* functions, and the
 * output hook writes the folded material (or P, or the fold's diagnostics) in
 * place of the colour.  No ray generation is restated, and the forced-step
 * replay comes with the oracle's render(): `force` imposes a kernel's recorded
 * step counts.  Built with the oracle's flags (-ffp-contract=off
 * -fno-fast-math) by sdf3d_amd/build.py build_materials_ref into
 * tests/build/libmaterials_ref.so; loaded by tests/materials_ref.py.
 */
#include <math.h>
#include <string.h>

#include "../include/sdf_abi.h"

enum { MAT_AMB = 0, MAT_DIF = 1, MAT_REF = 2, MAT_POINT = 3, MAT_INFO = 4 };

/* what one fold leaves: the blended components, the scene fold's final d,
 * the smallest |a - b| over the hard decisions after primitive 0, the
 * primitive of the largest weight, whether the result is a true mix, and the
 * last primitive's weight t */
typedef struct {
  float m[9];
  float d, min_gap, last_t;
  int owner, blended;
} mat_fold_out;

static _Thread_local mat_fold_out t_fold;
static _Thread_local float t_point[3];
static const sdf_material* g_materials;
static int g_what;

static void mat_capture(const sdf_scene* s, float x, float y, float z);
static void mat_write(float* px);

#define ORACLE_PIXEL_HOOK(lit) mat_capture(s, (float)P.x, (float)P.y, (float)P.z)
#define ORACLE_TERMS_HOOK(ao, dif, spec, x, ndl, sh) ((void)0)
#define ORACLE_PIXEL_OUT_HOOK(px) mat_write(px)

#include "../oracle/sdf_oracle.c"

/* The material fold at p: oracle_core.h scene_sdf's loop with the running
 * material beside the running distance. */
static void mat_fold(const sdf_scene* s, f32_v3 p, const sdf_material* M, mat_fold_out* o) {
  float d = INFINITY;
  double w[SDF_MAX_PRIMS] = {1.0};
  for (int c = 0; c < 3; c++) {
    o->m[c] = M[0].amb[c];
    o->m[3 + c] = M[0].dif[c];
    o->m[6 + c] = M[0].ref[c];
  }
  o->min_gap = INFINITY;
  o->last_t = 0.0f;
  for (int i = 0; i < s->count; i++) {
    const sdf_primitive* pr = &s->prims[i];
    float v;
    switch (pr->kind) {
      case SDF_PRIM_SPHERE: v = f32_sd_sphere(p, pr->p); break;
      case SDF_PRIM_PLANE: v = f32_sd_plane(p, pr->p); break;
      case SDF_PRIM_BOX: v = f32_sd_box(p, pr->p); break;
      case SDF_PRIM_ROUND_BOX: v = f32_sd_round_box(p, pr->p); break;
      case SDF_PRIM_TORUS: v = f32_sd_torus(p, pr->p); break;
      case SDF_PRIM_CAPSULE: v = f32_sd_capsule(p, pr->p); break;
      default: v = f32_sd_cylinder(p, pr->p); break;
    }
    const float k = pr->k;
    const int op = pr->op;
    const int smooth = op == SDF_OP_SMOOTH_UNION || op == SDF_OP_SMOOTH_SUBTRACT ||
                       op == SDF_OP_SMOOTH_INTERSECT;
    /* (a, b): the arguments scene_sdf hands to gmin / smin */
    const float a = (op == SDF_OP_UNION || op == SDF_OP_SMOOTH_UNION) ? d : -d;
    const float b = (op == SDF_OP_INTERSECT || op == SDF_OP_SMOOTH_INTERSECT) ? -v : v;
    float t;
    if (smooth) {
      const float h = f32_gmax(k - fabsf(a - b), 0) / k;   /* smin's own h */
      const float hh = h * h;
      const float q = hh * 0.5f;
      t = (b < a) ? 1.0f - q : q;
    } else {
      t = (b < a) ? 1.0f : 0.0f;
      if (i > 0) {
        const float gap = fabsf(a - b);
        if (gap < o->min_gap) o->min_gap = gap;
      }
    }
    const float Mi[9] = {M[i].amb[0], M[i].amb[1], M[i].amb[2], M[i].dif[0], M[i].dif[1],
                         M[i].dif[2], M[i].ref[0], M[i].ref[1], M[i].ref[2]};
    for (int c = 0; c < 9; c++) {
      if (t == 0.0f) continue;
      if (t == 1.0f) {
        o->m[c] = Mi[c];
      } else {
        const float diff = Mi[c] - o->m[c];
        const float step = t * diff;
        o->m[c] = o->m[c] + step;
      }
    }
    /* weights (diagnostics): the start value is materials[0] too */
    if (i > 0) {
      for (int j = 0; j < i; j++) w[j] *= 1.0 - (double)t;
      w[i] = (double)t;
    }
    o->last_t = t;
    switch (op) {
      case SDF_OP_UNION: d = f32_gmin(d, v); break;
      case SDF_OP_SMOOTH_UNION: d = f32_smin(d, v, k); break;
      case SDF_OP_SUBTRACT: d = f32_gmax(d, -v); break;
      case SDF_OP_INTERSECT: d = f32_gmax(d, v); break;
      case SDF_OP_SMOOTH_SUBTRACT: d = -f32_smin(-d, v, k); break;
      default: d = -f32_smin(-d, -v, k); break;
    }
  }
  o->d = d;
  o->owner = 0;
  for (int i = 1; i < s->count; i++)
    if (w[i] > w[o->owner]) o->owner = i;
  o->blended = s->count > 0 && w[o->owner] < 1.0;
}

static void mat_capture(const sdf_scene* s, float x, float y, float z) {
  t_point[0] = x;
  t_point[1] = y;
  t_point[2] = z;
  if (g_materials && s->kind == SDF_SCENE_PRIMITIVES)
    mat_fold(s, f32_mk(x, y, z), g_materials, &t_fold);
}

static void mat_write(float* px) {
  if (!g_materials) return;
  switch (g_what) {
    case MAT_AMB: case MAT_DIF: case MAT_REF:
      memcpy(px, t_fold.m + 3 * g_what, 3 * sizeof(float));
      px[3] = 1.0f;
      break;
    case MAT_POINT:
      memcpy(px, t_point, 3 * sizeof(float));
      px[3] = t_fold.d;
      break;
    default:
      px[0] = t_fold.min_gap;
      px[1] = (float)t_fold.owner;
      px[2] = (float)t_fold.blended;
      px[3] = t_fold.d;
      break;
  }
}

/* One plane of the fold per pixel of the fp32 oracle's frame (`what`: MAT_*),
 * [rows][W][4] floats:
 *   MAT_AMB / MAT_DIF / MAT_REF  the blended amb / dif / ref, 1
 *   MAT_POINT                    P.xyz, the fold's final d
 *   MAT_INFO                     min_gap, owner, blended (0 / 1), final d
 * `force` (may be NULL): per-pixel (primary, shadow) step counts to impose, as
 * sdf_oracle_replay takes them (a primary count of -2 skips the pixel).
 * Primitive scenes only; one call at a time. */
int sdf_materials_ref_render(const sdf_scene* s, const sdf_camera* c, const sdf_light* l,
                             const sdf_material* materials, int nmaterials,
                             const sdf_params* p, const sdf_tiling* t, const int* force,
                             int what, float* out, int nthreads) {
  if (!s || !materials || s->kind != SDF_SCENE_PRIMITIVES || nmaterials != s->count ||
      what < MAT_AMB || what > MAT_INFO)
    return SDF_E_INVALID_ARG;
  g_materials = materials;
  g_what = what;
  const int rc = render(0, s, c, l, &materials[0], p, t, out, 0, force, nthreads);
  g_materials = 0;
  return rc;
}

/* The fold at one point: out9 = the blended components, info5 = final d,
 * min_gap, owner, blended, the last primitive's t. */
int sdf_materials_ref_fold(const sdf_scene* s, const sdf_material* materials, int nmaterials,
                           float x, float y, float z, float* out9, float* info5) {
  if (!s || !materials || s->kind != SDF_SCENE_PRIMITIVES || nmaterials != s->count)
    return SDF_E_INVALID_ARG;
  mat_fold_out o;
  mat_fold(s, f32_mk(x, y, z), materials, &o);
  memcpy(out9, o.m, sizeof(o.m));
  info5[0] = o.d;
  info5[1] = o.min_gap;
  info5[2] = (float)o.owner;
  info5[3] = (float)o.blended;
  info5[4] = o.last_t;
  return SDF_OK;
}
