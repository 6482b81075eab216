/*
 * reflect_ref.c -- TEST INFRASTRUCTURE ONLY: the reference of mirror
 * reflections (include/sdf_abi.h "Reflections", sdf_render_reflect) over the
 * CPU oracle.  It includes the oracle's translation unit, the way
 * materials_ref.c does.  The oracle's own render loop generates every pixel's
 * camera position and ray; its output hook hands them to ref_walk, which
 * walks the pixel's path layer by layer with the oracle's own shade_pixel
 * (f32_shade_pixel shades a fragment for an arbitrary eye and ray), once per
 * light.  The instrumentation hooks inside shade_pixel capture P, N, d and
 * the light's terms; the material fold at P is materials_ref.c's
 * (sdf_materials_ref_fold, linked from libmaterials_ref.so).  No ray
 * generation and no march is restated: the only arithmetic of its own is the
 * contract's next ray and weights, written with the oracle's vector helpers.
 * What a layer's colour and the composite are is stated in NumPy
 * (tests/reflect_ref.py) from the planes this file records.  Built with the
 * oracle's flags by sdf3d_amd/build.py build_reflect_ref into
 * tests/build/libreflect_ref.so.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../include/sdf_abi.h"

/* floats recorded per pixel and layer (tests/reflect_ref.py names them) */
enum {
  RF_ALIVE = 0,   /* 1: the path reached this layer                         */
  RF_O = 1,       /* the layer's eye                                          */
  RF_D = 4,       /* and ray                                                  */
  RF_P = 7,
  RF_N = 10,
  RF_DIST = 13,   /* d: the primary march's distance                          */
  RF_AO = 14,
  RF_MAT = 15,    /* the blended amb, dif, ref (9)                            */
  RF_W = 24,      /* W_j                                                      */
  RF_SP = 27,     /* the primary march's step count                           */
  RF_SS = 28,     /* light i's shadow step count (8)                          */
  RF_DIF = 36,    /* light i's dif (8)                                        */
  RF_X = 44,      /* light i's x = max(N.H, 0) (8)                            */
  RF_OWN = 52,    /* shade_pixel's own colour with the blended material, light 0 */
  RF_FLOATS = 56
};
/* ints per pixel and layer of a forced replay: primary, shadow of light i */
enum { RF_FORCE = 1 + SDF_MAX_LIGHTS };

static _Thread_local float t_P[3], t_N[3], t_d, t_ao, t_dif, t_x;

static void ref_walk(const sdf_scene* s, const sdf_params* pa, size_t o, float cx, float cy,
                     float cz, float rx, float ry, float rz);

#define ORACLE_PIXEL_HOOK(lit)                                                        \
  (t_P[0] = (float)P.x, t_P[1] = (float)P.y, t_P[2] = (float)P.z, t_N[0] = (float)N.x, \
   t_N[1] = (float)N.y, t_N[2] = (float)N.z, t_d = (float)d)
#define ORACLE_TERMS_HOOK(ao, dif, spec, x, ndl, sh) \
  (t_ao = (float)(ao), t_dif = (float)(dif), t_x = (float)(x))
#define ORACLE_PIXEL_OUT_HOOK(px)                                                          \
  ref_walk(s, pa, o, (float)cam.x, (float)cam.y, (float)cam.z, (float)ray.x, (float)ray.y, \
           (float)ray.z)

#include "../oracle/sdf_oracle.c"

/* tests/materials_ref.c (libmaterials_ref.so) */
int sdf_materials_ref_fold(const sdf_scene* s, const sdf_material* materials, int nmaterials,
                           float x, float y, float z, float* out9, float* info5);

static const sdf_light* g_lights;
static int g_nlights;
static const sdf_material* g_materials;
static int g_nmaterials;
static int g_bounces;
static float g_strength;
static const int* g_force;
static float* g_out;

static void ref_walk(const sdf_scene* s, const sdf_params* pa, size_t o, float cx, float cy,
                     float cz, float rx, float ry, float rz) {
  if (!g_out) return;
  const int layers = g_bounces + 1;
  float* base = g_out + o * (size_t)layers * RF_FLOATS;
  memset(base, 0, sizeof(float) * (size_t)layers * RF_FLOATS);
  f32_v3 O = f32_mk(cx, cy, cz), D = f32_mk(rx, ry, rz);
  float W[3] = {1.0f, 1.0f, 1.0f};
  for (int j = 0; j < layers; j++) {
    float* r = base + (size_t)j * RF_FLOATS;
    const int* fo = g_force ? g_force + (o * (size_t)layers + (size_t)j) * RF_FORCE : 0;
    float px[4];
    int32_t st[2];
    for (int i = 0; i < g_nlights; i++) {
      int32_t f2[2] = {fo ? fo[0] : -1, fo ? fo[1 + i] : -1};
      f32_shade_pixel(s, &g_lights[i], &g_materials[0], pa, O, D, px, st, fo ? f2 : 0);
      r[RF_SS + i] = (float)st[1];
      r[RF_DIF + i] = t_dif;
      r[RF_X + i] = t_x;
    }
    /* P, N, d, ao and the primary count do not depend on the light */
    r[RF_ALIVE] = 1.0f;
    r[RF_O] = O.x; r[RF_O + 1] = O.y; r[RF_O + 2] = O.z;
    r[RF_D] = D.x; r[RF_D + 1] = D.y; r[RF_D + 2] = D.z;
    memcpy(r + RF_P, t_P, sizeof(t_P));
    memcpy(r + RF_N, t_N, sizeof(t_N));
    r[RF_DIST] = t_d;
    r[RF_AO] = t_ao;
    r[RF_SP] = (float)st[0];
    memcpy(r + RF_W, W, sizeof(W));
    /* the blended material at P (a Mandelbulb has materials[0]) */
    sdf_material m = g_materials[0];
    if (s->kind == SDF_SCENE_PRIMITIVES) {
      float m9[9], info[5];
      sdf_materials_ref_fold(s, g_materials, g_nmaterials, t_P[0], t_P[1], t_P[2], m9, info);
      memcpy(m.amb, m9, 3 * sizeof(float));
      memcpy(m.dif, m9 + 3, 3 * sizeof(float));
      memcpy(m.ref, m9 + 6, 3 * sizeof(float));
    }
    memcpy(r + RF_MAT, m.amb, 3 * sizeof(float));
    memcpy(r + RF_MAT + 3, m.dif, 3 * sizeof(float));
    memcpy(r + RF_MAT + 6, m.ref, 3 * sizeof(float));
    /* the oracle's own colour of this fragment with the blended material
     * under light 0 (what C_j is for one plain light) */
    {
      const f32_v3 P = f32_mk(t_P[0], t_P[1], t_P[2]), N = f32_mk(t_N[0], t_N[1], t_N[2]);
      const float d = t_d;
      int32_t f2[2] = {fo ? fo[0] : -1, fo ? fo[1] : -1};
      f32_shade_pixel(s, &g_lights[0], &m, pa, O, D, px, st, fo ? f2 : 0);
      memcpy(r + RF_OWN, px, 3 * sizeof(float));
      /* W_(j+1) and the end of the path */
      for (int c = 0; c < 3; c++) {
        const float k = g_strength * m.ref[c];
        W[c] = W[c] * k;
      }
      if (j == g_bounces || d > pa->max_dist || (W[0] == 0.0f && W[1] == 0.0f && W[2] == 0.0f))
        break;
      /* the next ray: D mirrored at N, from the shadow march's origin
       * (oracle_core.h shade_pixel `o`) */
      const float nd = f32_dot(N, D);
      const float s2 = 2.0f * nd;
      D = f32_normalize(f32_mk(D.x - s2 * N.x, D.y - s2 * N.y, D.z - s2 * N.z));
      const float off = pa->shadow_offset, eps = pa->eps;
      O = f32_mk(P.x + N.x * off * eps, P.y + N.y * off * eps, P.z + N.z * off * eps);
    }
  }
}

/* Every pixel's path: out is [rows][W][bounces + 1][RF_FLOATS] floats (layers
 * the path did not reach are zero), in the packed row order of tiling `t`.
 * `force` (may be NULL): [rows][W][bounces + 1][RF_FORCE] step counts to
 * impose on the layers the reference itself reaches (primary, then light i's
 * shadow march).  One call at a time. */
int sdf_reflect_ref_render(const sdf_scene* s, const sdf_camera* c, const sdf_light* lights,
                           int nlights, const sdf_material* materials, int nmaterials,
                           int bounces, float strength, const sdf_params* p, const sdf_tiling* t,
                           const int* force, float* out, int nthreads) {
  if (!s || !lights || !materials || !out || nlights < 1 || nlights > SDF_MAX_LIGHTS ||
      bounces < 0 || bounces > SDF_MAX_BOUNCES ||
      nmaterials != (s->kind == SDF_SCENE_PRIMITIVES ? s->count : 1))
    return SDF_E_INVALID_ARG;
  g_lights = lights;
  g_nlights = nlights;
  g_materials = materials;
  g_nmaterials = nmaterials;
  g_bounces = bounces;
  g_strength = strength;
  g_force = force;
  g_out = out;
  /* the oracle's render loop forms each pixel's camera and ray; its own
   * colour goes to a scratch pixel row by row */
  float* scratch = 0;
  int rc = SDF_E_INVALID_ARG;
  if (p && p->width > 0 && p->height > 0) {
    scratch = (float*)malloc(sizeof(float) * 4 * (size_t)p->width * (size_t)p->height);
    if (scratch) rc = render(0, s, c, &lights[0], &materials[0], p, t, scratch, 0, 0, nthreads);
  }
  free(scratch);
  g_out = 0;
  g_force = 0;
  return rc;
}

int sdf_reflect_ref_floats(void) { return RF_FLOATS; }
