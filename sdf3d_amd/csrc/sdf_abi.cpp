// sdf_abi.cpp -- host side of the C-ABI declared in include/sdf_abi.h.
//
// Replaces what the reference does around `gl->plot(sh, proj_mode)`
// (/root/reference/Code/src/main.cpp:95): it takes the per-frame uniforms
// (the shader's V_mat and AR, voxel_fragment.frag:5-7) plus the scene, light
// and material that the reference hard-codes in the shader
// (voxel_fragment.frag:178-189), hoists the uniform-only arithmetic the shader
// repeats per pixel (inverse(V_mat) at :180 and :192, camera.pos at :180, the
// focal term at :191), and launches one HIP kernel over the requested rows.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

#include "../../include/sdf_abi.h"
#include "host_api.h"
#include "kernel_args.h"

// Layout contract with the ctypes mirror (sdf3d_amd/abi.py STRUCT_SIZES).
static_assert(sizeof(sdf_primitive) == 64, "sdf_primitive layout");
static_assert(sizeof(sdf_scene) == 8 + 64 * SDF_MAX_PRIMS + 32, "sdf_scene layout");
static_assert(sizeof(sdf_camera) == 88, "sdf_camera layout");
static_assert(sizeof(sdf_light) == 32, "sdf_light layout");
static_assert(sizeof(sdf_material) == 40, "sdf_material layout");
static_assert(sizeof(sdf_params) == 80, "sdf_params layout");
static_assert(sizeof(sdf_tiling) == 24, "sdf_tiling layout");
static_assert(sizeof(sdf_driver_config) == 36, "sdf_driver_config layout");
static_assert(sizeof(sdf_hits) == 32, "sdf_hits layout");

namespace sdf {

int tiling_run(const sdf_tiling& t) { return t.block_run > 1 ? t.block_run : 1; }
int tiling_step(const sdf_tiling& t) { return t.run_step > 1 ? t.run_step : 1; }
int tiling_gap_rows(const sdf_tiling& t) { return (tiling_step(t) - 1) * t.block_rows; }

int count_rows(int height, const sdf_tiling& t) {
  if (t.block_rows <= 0 || t.block_stride <= 0 || t.first_block < 0 || height < 0 ||
      t.block_run < 0 || t.run_step < 0 ||
      (long long)(tiling_run(t) - 1) * tiling_step(t) >= t.block_stride ||
      (t.flags & ~SDF_TILING_FRAME_ROWS) != 0)
    return SDF_E_INVALID_ARG;
  // spaced runs keep every 8-row tile of packed rows inside one block (the
  // kernels then find a tile's block once per wave)
  if (tiling_step(t) > 1 && t.block_rows % 8 != 0) return SDF_E_INVALID_ARG;
  // every period contributes its run of blocks, cut at the frame's last row
  long long rows = 0;
  const long long B = t.block_rows;
  for (long long b0 = t.first_block; b0 * B < height; b0 += t.block_stride)
    for (long long j = 0; j < tiling_run(t); ++j) {
      const long long b = b0 + j * tiling_step(t);
      if (b * B < height) rows += std::min<long long>((b + 1) * B, height) - b * B;
    }
  return (int)rows;
}

}  // namespace sdf

namespace {

// Inverse of a column-major 4x4 matrix via 2x2 sub-determinants, in double,
// rounded once to float.  GLSL's inverse() precision is unspecified; this is
// the correctly rounded exact inverse for all but pathological inputs.
bool invert_view(const float* mf, float* out) {
  double m[16];
  for (int i = 0; i < 16; ++i) m[i] = mf[i];
  // element (row r, col c) of a column-major matrix is m[c*4 + r]
  auto e = [&](int r, int c) { return m[c * 4 + r]; };
  const double s0 = e(0, 0) * e(1, 1) - e(1, 0) * e(0, 1);
  const double s1 = e(0, 0) * e(1, 2) - e(1, 0) * e(0, 2);
  const double s2 = e(0, 0) * e(1, 3) - e(1, 0) * e(0, 3);
  const double s3 = e(0, 1) * e(1, 2) - e(1, 1) * e(0, 2);
  const double s4 = e(0, 1) * e(1, 3) - e(1, 1) * e(0, 3);
  const double s5 = e(0, 2) * e(1, 3) - e(1, 2) * e(0, 3);
  const double c5 = e(2, 2) * e(3, 3) - e(3, 2) * e(2, 3);
  const double c4 = e(2, 1) * e(3, 3) - e(3, 1) * e(2, 3);
  const double c3 = e(2, 1) * e(3, 2) - e(3, 1) * e(2, 2);
  const double c2 = e(2, 0) * e(3, 3) - e(3, 0) * e(2, 3);
  const double c1 = e(2, 0) * e(3, 2) - e(3, 0) * e(2, 2);
  const double c0 = e(2, 0) * e(3, 1) - e(3, 0) * e(2, 1);
  const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
  if (det == 0.0 || !std::isfinite(det)) return false;
  double inv[4][4];  // inv[r][c]
  inv[0][0] = (e(1, 1) * c5 - e(1, 2) * c4 + e(1, 3) * c3);
  inv[0][1] = (-e(0, 1) * c5 + e(0, 2) * c4 - e(0, 3) * c3);
  inv[0][2] = (e(3, 1) * s5 - e(3, 2) * s4 + e(3, 3) * s3);
  inv[0][3] = (-e(2, 1) * s5 + e(2, 2) * s4 - e(2, 3) * s3);
  inv[1][0] = (-e(1, 0) * c5 + e(1, 2) * c2 - e(1, 3) * c1);
  inv[1][1] = (e(0, 0) * c5 - e(0, 2) * c2 + e(0, 3) * c1);
  inv[1][2] = (-e(3, 0) * s5 + e(3, 2) * s2 - e(3, 3) * s1);
  inv[1][3] = (e(2, 0) * s5 - e(2, 2) * s2 + e(2, 3) * s1);
  inv[2][0] = (e(1, 0) * c4 - e(1, 1) * c2 + e(1, 3) * c0);
  inv[2][1] = (-e(0, 0) * c4 + e(0, 1) * c2 - e(0, 3) * c0);
  inv[2][2] = (e(3, 0) * s4 - e(3, 1) * s2 + e(3, 3) * s0);
  inv[2][3] = (-e(2, 0) * s4 + e(2, 1) * s2 - e(2, 3) * s0);
  inv[3][0] = (-e(1, 0) * c3 + e(1, 1) * c1 - e(1, 2) * c0);
  inv[3][1] = (e(0, 0) * c3 - e(0, 1) * c1 + e(0, 2) * c0);
  inv[3][2] = (-e(3, 0) * s3 + e(3, 1) * s1 - e(3, 2) * s0);
  inv[3][3] = (e(2, 0) * s3 - e(2, 1) * s1 + e(2, 2) * s0);
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) out[c * 4 + r] = static_cast<float>(inv[r][c] / det);
  return true;
}

// the ops that blend over a radius k
bool smooth_op(int op) {
  return op == SDF_OP_SMOOTH_UNION || op == SDF_OP_SMOOTH_SUBTRACT || op == SDF_OP_SMOOTH_INTERSECT;
}

bool finite3(const float* v) {
  return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
}

using sdf::count_rows;

const sdf_tiling kWholeFrame = {8, 0, 1, 0, 1, 1};

// Per-frame preparation of the primitive parameter blocks the kernels read
// (layouts in prims.inc).  Every derived value is computed in fp32
// with the operation order the oracle uses per evaluation (oracle_core.h), so
// the exact-precision kernel stays bit-identical; 1/x values are only used by
// the fast-precision kernel.
void prepare_prims(const sdf_scene& s, sdf_primitive* out) {
  std::memcpy(out, s.prims, sizeof(s.prims));
  for (int i = 0; i < s.count; ++i) {
    const sdf_primitive& in = s.prims[i];
    sdf_primitive& o = out[i];
    o.reserved = in.k > 0.0f ? 1.0f / in.k : 0.0f;
    o.p[11] = in.k * 0.25f;  // smooth-min k/4 (fast precision)
    // exact precision's smooth-min division n / k (prims.inc smin,
    // cr_math.h smin_h / div_scaled): sc = 2^s with k sc in [0.5, 1) (s <=
    // 127, so a denormal k lands in [2^-22, 1)), and RN(1/(k sc)) by an IEEE
    // division.  k sc < 1: smin_h's clamp to [0, 1] is its max(., 0) alone
    float sc = 1.0f, ks = 1.0f;
    if (in.k > 0.0f && std::isfinite(in.k)) {
      int e = 0;
      (void)std::frexp(in.k, &e);                 // k = m 2^e, m in [0.5, 1)
      sc = std::ldexp(1.0f, std::min(-e, 127));
      ks = in.k * sc;                             // exact
    }
    o.p[9] = sc;
    o.p[10] = 1.0f / ks;
    // the prepared block's k slot carries k sc for the exact kernel (its
    // smooth-min reads k/4 from p[11] and k sc here; nothing else reads it)
    o.k = ks;
    const float* q = in.p;
    float* p = o.p;
    switch (in.kind) {
      case SDF_PRIM_ROUND_BOX: {
        const float r = q[6];
        p[3] = q[3] - r;
        p[4] = q[4] - r;
        p[5] = q[5] - r;
        p[6] = r;
        break;
      }
      case SDF_PRIM_CAPSULE: {
        const float bax = q[3] - q[0], bay = q[4] - q[1], baz = q[5] - q[2];
        const float baba = bax * bax + bay * bay + baz * baz;
        p[3] = bax;
        p[4] = bay;
        p[5] = baz;
        p[6] = q[6];
        p[7] = baba;
        p[8] = 1.0f / baba;
        break;
      }
      default:
        break;
    }
  }
}

// A small sphere containing the n spheres (c_i, r_i): the centre C minimises
// RC(C) = max_i |c_i - C| + r_i, which is convex in C.  Any C gives a valid
// bound; the search only makes it tighter (subgradient steps towards the
// farthest sphere with diminishing length from the centroid, and the
// two-sphere balls of every pair, keeping the best).  The tighter the
// cluster sphere, the more often the culling and the shadow march's lit
// tail (scenes.inc, trace.inc) skip it.  Cached per primitive list: sdf_render
// prepares a plan per call.
static double sphere_radius_at(const double (*c)[3], const double* r, int n, const double* C) {
  double R = 0;
  for (int i = 0; i < n; ++i) {
    const double dx = c[i][0] - C[0], dy = c[i][1] - C[1], dz = c[i][2] - C[2];
    R = std::max(R, std::sqrt(dx * dx + dy * dy + dz * dz) + r[i]);
  }
  return R;
}
static double cluster_sphere(const double (*c)[3], const double* r, int n, double* C) {
  thread_local double key[SDF_MAX_PRIMS * 4 + 1] = {-1};
  thread_local double kC[3], kR = 0;
  double k[SDF_MAX_PRIMS * 4 + 1] = {(double)n};
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < 3; ++j) k[1 + 4 * i + j] = c[i][j];
    k[4 + 4 * i] = r[i];
  }
  if (std::memcmp(k, key, sizeof(double) * (1 + 4 * n)) == 0) {
    std::memcpy(C, kC, sizeof(kC));
    return kR;
  }
  double B[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) B[j] += c[i][j] / n;
  double RB = sphere_radius_at(c, r, n, B);
  // the ball of each pair, through both spheres' far points
  for (int i = 0; i < n; ++i)
    for (int m = i + 1; m < n; ++m) {
      double u[3], L = 0;
      for (int j = 0; j < 3; ++j) { u[j] = c[m][j] - c[i][j]; L += u[j] * u[j]; }
      L = std::sqrt(L);
      if (!(L > 0)) continue;
      const double off = 0.5 * (L + r[m] - r[i]);
      double T[3];
      for (int j = 0; j < 3; ++j) T[j] = c[i][j] + u[j] / L * off;
      const double RT = sphere_radius_at(c, r, n, T);
      if (RT < RB) { RB = RT; std::memcpy(B, T, sizeof(B)); }
    }
  // subgradient descent from the best so far
  double X[3];
  std::memcpy(X, B, sizeof(X));
  const double step0 = 0.25 * RB;
  for (int it = 0; it < 2000; ++it) {
    int far = 0;
    double best = -1, dist = 0;
    for (int i = 0; i < n; ++i) {
      const double dx = c[i][0] - X[0], dy = c[i][1] - X[1], dz = c[i][2] - X[2];
      const double d = std::sqrt(dx * dx + dy * dy + dz * dz);
      if (d + r[i] > best) { best = d + r[i]; far = i; dist = d; }
    }
    if (best < RB) { RB = best; std::memcpy(B, X, sizeof(B)); }
    if (!(dist > 0)) break;
    const double h = step0 / (1.0 + it);
    for (int j = 0; j < 3; ++j) X[j] += (c[far][j] - X[j]) / dist * h;
  }
  std::memcpy(key, k, sizeof(double) * (1 + 4 * n));
  std::memcpy(kC, B, sizeof(kC));
  kR = RB;
  std::memcpy(C, B, sizeof(kC));
  return RB;
}

// Host-only constants of the culling margins (no kernel reads them).  The
// cached gaps (scenes.inc FixedScene::march) compare computed path
// points o + D t, each rounded by up to sqrt 3 2^-24 (|D t|_inf + |p|_inf);
// at most four such points lie between a stored gap and its use, and
// 4 sqrt 3 2^-24 < 2^-21: kCullPath holds twice that.
constexpr double kCullPath = 0x1p-20;
constexpr double kCullMaxCoord = 0x1p22;

// Bounding spheres and the cluster bound read by the kernels' culling
// (kernel_args.h "exact bounding-volume culling").  Radii are computed in
// double, around the fp32 centre the kernels read, and rounded up.
//
// `cached`: the plan's kernel keeps gaps along a path (FixedScene).  Each
// bound's absolute margin is then kCullAbs + kCullPath (|c|_inf + R + k +
// reach), the second term covering the fp32 rounding of the path points
// o + D t between which a gap is carried (DESIGN.md "Culling margins at large
// coordinates"); `reach` is the longest ray segment of the plan, its
// max_dist.  The generic kernel makes every test afresh at the point it
// evaluates and needs no such term: sdf_scene_bounds reports its bounds.
// Returns false, with cluster_first = count, when the cullable primitives
// reach beyond kCullMaxCoord, where neither argument is made: the caller
// must then take the unculled path.
bool prepare_bounds(const sdf_scene& s, sdf::KernelArgs& a, bool exact = false,
                    bool cached = false, double reach = 0.0) {
  std::memset(a.bound, 0, sizeof(a.bound));
  a.cluster_first = s.count;
  double cen[SDF_MAX_PRIMS][3], rad[SDF_MAX_PRIMS];
  bool cull[SDF_MAX_PRIMS];
  double span = 0;   // the largest |c|_inf + R + k of a cullable primitive
  for (int i = 0; i < s.count; ++i) {
    const sdf_primitive& pr = s.prims[i];
    const float* q = pr.p;
    double c[3] = {q[0], q[1], q[2]}, R = 0;
    switch (pr.kind) {
      case SDF_PRIM_SPHERE: R = q[3]; break;
      case SDF_PRIM_BOX: R = std::sqrt(double(q[3]) * q[3] + double(q[4]) * q[4] + double(q[5]) * q[5]); break;
      case SDF_PRIM_ROUND_BOX: {
        // the box (b - r) rounded by r (prims.inc sd_round_box; a
        // negative b - r only shrinks the shape: box_core falls with e)
        double e2 = 0;
        for (int j = 3; j < 6; ++j) {
          const double e = std::max(double(q[j]) - q[6], 0.0);
          e2 += e * e;
        }
        R = std::sqrt(e2) + std::fabs(double(q[6]));
        break;
      }
      case SDF_PRIM_TORUS: R = double(q[3]) + q[4]; break;
      case SDF_PRIM_CAPSULE: {
        // the sphere about the midpoint, enlarged by what the midpoint
        // loses when it is rounded to the fp32 centre the kernels read: up to
        // half an ulp of the coordinates per axis, whatever the capsule's size
        double half2 = 0, off2 = 0;
        for (int j = 0; j < 3; ++j) {
          const double m = 0.5 * (double(q[j]) + q[3 + j]), h = 0.5 * (double(q[3 + j]) - q[j]);
          c[j] = double(float(m));
          half2 += h * h;
          off2 += (c[j] - m) * (c[j] - m);
        }
        R = std::sqrt(half2) + q[6] + std::sqrt(off2);
        break;
      }
      case SDF_PRIM_CYLINDER: R = std::sqrt(double(q[3]) * q[3] + double(q[4]) * q[4]); break;
      default: R = 0; break;
    }
    R = std::fabs(R) * (1.0 + 1e-6) + 1e-6;
    const int kind = sdf::prim_kind(pr);
    cull[i] = sdf::cullable(kind, pr.op);
    const double k = pr.op == SDF_OP_SMOOTH_UNION ? pr.k : 0.0;
    for (int j = 0; j < 3; ++j) { cen[i][j] = c[j]; a.bound[i][j] = float(c[j]); }
    rad[i] = R;
    const double reachi =
        std::max({std::fabs(c[0]), std::fabs(c[1]), std::fabs(c[2])}) + R + k;
    if (cull[i]) span = std::max(span, reachi);
    const double margin = sdf::kCullAbs + (cached ? kCullPath * (reachi + reach) : 0.0);
    // K' = (k + R + margin) / (1 - kCullRel), rounded up (scenes.inc wave_near)
    a.bound[i][3] = float((k + R + margin) / (1.0 - sdf::kCullRel) * (1.0 + 1e-6));
    // exact kernel (the prepared block's `reserved`, unused there): the
    // offset of the gap an evaluated primitive's own value leaves in the
    // culling cache, k + margin + 1e-4 R (scenes.inc step_cached),
    // rounded up
    if (exact && sdf::cullable(kind, pr.op))
      a.prims[i].reserved = float((k + margin + 1e-4 * R) * (1.0 + 1e-6));
  }
  int first = s.count;
  while (first > 0 && cull[first - 1]) --first;
  if (first < s.count && !(span + reach <= kCullMaxCoord)) return false;
  a.cluster_first = first;
  if (first < s.count) {
    double C[3];
    cluster_sphere(cen + first, rad + first, s.count - first, C);
    for (int j = 0; j < 3; ++j) C[j] = double(float(C[j]));   // the centre the kernel reads
    const double RC = sphere_radius_at(cen + first, rad + first, s.count - first, C);
    double kmax = 0;
    for (int i = first; i < s.count; ++i)
      if (s.prims[i].op == SDF_OP_SMOOTH_UNION) kmax = std::max(kmax, double(s.prims[i].k));
    for (int j = 0; j < 3; ++j) a.cluster[j] = float(C[j]);
    const double cmax = std::max({std::fabs(C[0]), std::fabs(C[1]), std::fabs(C[2])});
    const double margin =
        sdf::kCullAbs + (cached ? kCullPath * (cmax + RC + kmax + reach) : 0.0);
    a.cluster[3] = float((kmax + RC * (1.0 + 1e-6) + 1e-6 + margin) /
                         (1.0 - sdf::kCullRel) * (1.0 + 1e-6));
  }
  return true;
}

}  // namespace

namespace sdf {

// (kind, op) sequence of a primitive scene, the compile-time signature of a
// FixedScene kernel (an upward plane through its own kind, kPrimPlaneY)
int scene_signature(const sdf_scene& scene, int* sig) {
  const int n = scene.count;
  for (int i = 0; i < n; ++i) sig[i] = SDF_KO(prim_kind(scene.prims[i]), scene.prims[i].op);
  return n;
}

int select_variant(const sdf_scene& scene) {
  if (scene.kind == SDF_SCENE_MANDELBULB) return kVariantBulb;
  int sig[SDF_MAX_PRIMS];
  const int n = scene_signature(scene, sig);
  auto match = [&](std::initializer_list<int> v) {
    if ((int)v.size() != n) return false;
    int i = 0;
    for (int k : v)
      if (sig[i++] != k) return false;
    return true;
  };
#define SDF_MATCH(id, ...) \
  if (match({__VA_ARGS__})) return id;
  SDF_FIXED_VARIANTS(SDF_MATCH)
#undef SDF_MATCH
  return kVariantGeneric;
}

}  // namespace sdf

// ---- a request's rules (sdf_abi.h), part by part ------------------------------
namespace {

// Working range of the kernels: every coordinate, size and distance at most
// 1e15 in magnitude (and capsules of positive length), so that no square,
// dot product or distance the scene evaluation forms overflows -- every
// primitive value is then finite and the accumulated scene distance is never
// NaN, which the exact kernel's hardware minimum relies on (prims.inc
// smin<HW>).
constexpr float kMaxCoord = 1e15f;
constexpr float kMinCapsule2 = 0x1p-30f;
constexpr float kMaxCapsule2 = 0x1p30f;

// params and tiling
int validate_params(const sdf_params& p, const sdf_tiling* tiling) {
  if (p.width <= 0 || p.height <= 0 || p.width > 65536 || p.height > 65536)
    return SDF_E_INVALID_ARG;
  // sub-samples per axis: 0 and 1 are one sample per pixel.  The sub-sample
  // frame S W x S H is what the kernels index (cr_math.h div_refined: a quad
  // numerator below 2^17 over at most 2^16), and its tiling's block_rows are
  // S times the request's
  if (p.samples != 0 && p.samples != 1 && p.samples != 2 && p.samples != 4)
    return SDF_E_INVALID_ARG;
  if (p.samples > 1) {
    if (p.samples * (long long)p.width > 65536 || p.samples * (long long)p.height > 65536)
      return SDF_E_INVALID_ARG;
    if (tiling && tiling->block_rows > INT32_MAX / p.samples) return SDF_E_INVALID_ARG;
  }
  if (p.max_steps < 0 || p.max_steps > (1 << 24)) return SDF_E_INVALID_ARG;
  // every length the marches add to a coordinate stays in the working range
  // (kMaxCoord): normal_eps^2 and the AO tap lengths must not overflow,
  // which the exact kernels' one-compare cr_sqrt guard relies on
  for (float v : {p.max_dist, p.eps, p.shadow_k, p.normal_eps, p.shadow_offset})
    if (!(std::fabs(v) <= kMaxCoord)) return SDF_E_INVALID_ARG;
  if (p.flags & SDF_FLAG_AO)
    for (float v : {p.ao_step, p.ao_base, p.ao_falloff, p.ao_strength})
      if (!(std::fabs(v) <= kMaxCoord)) return SDF_E_INVALID_ARG;
  if (p.flags & ~(SDF_FLAG_SHADOW | SDF_FLAG_AO)) return SDF_E_INVALID_ARG;
  if (p.normal_mode != SDF_NORMAL_CENTRAL && p.normal_mode != SDF_NORMAL_TETRA)
    return SDF_E_INVALID_ARG;
  if (p.precision != SDF_PRECISION_EXACT && p.precision != SDF_PRECISION_FAST)
    return SDF_E_INVALID_ARG;
  if (p.dispatch < SDF_DISPATCH_AUTO || p.dispatch > SDF_DISPATCH_UNCULLED)
    return SDF_E_INVALID_ARG;
  if (p.output_format != SDF_FORMAT_TILES && sdf_format_bytes(p.output_format) < 0)
    return SDF_E_INVALID_ARG;
  if ((p.flags & SDF_FLAG_AO) && (p.ao_taps < 0 || p.ao_taps > sdf::kMaxAoTaps))
    return SDF_E_INVALID_ARG;
  if (count_rows(p.height, tiling ? *tiling : kWholeFrame) < 0) return SDF_E_INVALID_ARG;
  if (tiling && (tiling->flags & SDF_TILING_FRAME_ROWS) && p.output_format == SDF_FORMAT_TILES)
    return SDF_E_INVALID_ARG;   // a stream is made of packed tiles
  return SDF_OK;
}

int validate_scene(const sdf_scene& scene) {
  if (scene.kind == SDF_SCENE_PRIMITIVES) {
    if (scene.count < 0 || scene.count > SDF_MAX_PRIMS) return SDF_E_INVALID_ARG;
    for (int i = 0; i < scene.count; ++i) {
      const sdf_primitive& pr = scene.prims[i];
      if (pr.kind < 0 || pr.kind >= SDF_PRIM_KIND_COUNT) return SDF_E_INVALID_ARG;
      if (pr.op < 0 || pr.op >= SDF_OP_COUNT) return SDF_E_INVALID_ARG;
      // a smooth blend radius in [2^-64, 1e15]: the exact smooth-min's
      // h h (k/4) relies on the lower end (prims.inc smin)
      if (smooth_op(pr.op) && !(pr.k >= 0x1p-64f && pr.k <= kMaxCoord)) return SDF_E_INVALID_ARG;
      for (float v : pr.p)
        if (!std::isfinite(v) || std::fabs(v) > kMaxCoord) return SDF_E_INVALID_ARG;
      if (pr.kind == SDF_PRIM_CAPSULE) {
        // a segment of length in [2^-15, 2^15): dot(ba, ba), computed as the
        // kernels do, in [2^-30, 2^30) -- the exact kernel's Markstein
        // division of h = dot(pa, ba) / dot(ba, ba) (prims.inc
        // sd_capsule) needs its divisor there
        const float bax = pr.p[3] - pr.p[0], bay = pr.p[4] - pr.p[1], baz = pr.p[5] - pr.p[2];
        const float baba = bax * bax + bay * bay + baz * baz;
        if (!(baba >= kMinCapsule2 && baba < kMaxCapsule2)) return SDF_E_INVALID_ARG;
      }
    }
    return SDF_OK;
  }
  if (scene.kind != SDF_SCENE_MANDELBULB) return SDF_E_INVALID_ARG;
  // local coordinates (p - c) * RN(1/scale) stay finite: |p - c| <= ~3e15
  // and 1/scale <= 1e15, so the exact kernel's Markstein steps (unbounded
  // above, BulbScene::local) never see an overflowing product
  if (!(scene.bulb_scale >= 1.0f / kMaxCoord && scene.bulb_scale <= kMaxCoord))
    return SDF_E_INVALID_ARG;
  for (float v : scene.bulb_center)
    if (!(std::fabs(v) <= kMaxCoord)) return SDF_E_INVALID_ARG;
  if (scene.bulb_iterations < 1 || scene.bulb_iterations > 64) return SDF_E_INVALID_ARG;
  // bailout in (0, 2^32]: its square stays finite, so every iteration's
  // x^2 + z^2 <= m <= bailout^2 is finite (the exact kernel's 1 / sqrt of it,
  // kmath.inc frsqrt, relies on that)
  if (!(scene.bulb_bailout > 0.0f && scene.bulb_bailout <= 4294967296.0f))
    return SDF_E_INVALID_ARG;
  return SDF_OK;
}

// the lights' own rules: the count, the flags, every position in the working
// range; a colour is an arbitrary finite factor (negative ones included)
int validate_lights(const sdf_light* lights, int32_t n, int32_t flags) {
  if (!lights || n < 1 || n > SDF_MAX_LIGHTS) return SDF_E_INVALID_ARG;
  if (flags & ~SDF_LIGHTS_COLOR) return SDF_E_INVALID_ARG;
  for (int i = 0; i < n; ++i) {
    for (float v : lights[i].pos)
      if (!(std::fabs(v) <= kMaxCoord)) return SDF_E_INVALID_ARG;
    if ((flags & SDF_LIGHTS_COLOR) && !finite3(lights[i].color)) return SDF_E_INVALID_ARG;
  }
  return SDF_OK;
}

int validate_reflect(const sdf_reflect* r) {
  if (!r) return SDF_E_INVALID_ARG;
  if (r->bounces < 0 || r->bounces > SDF_MAX_BOUNCES) return SDF_E_INVALID_ARG;
  if (r->layer < -1 || r->layer > r->bounces) return SDF_E_INVALID_ARG;
  if (r->flags & ~SDF_REFLECT_WEIGHT) return SDF_E_INVALID_ARG;
  if ((r->flags & SDF_REFLECT_WEIGHT) && r->layer < 0) return SDF_E_INVALID_ARG;
  if (!std::isfinite(r->strength)) return SDF_E_INVALID_ARG;
  return SDF_OK;
}

// sdf_environment's own rules (sdf_abi.h "Environment"); fields of a feature
// whose flag is off are not looked at
int validate_environment(const sdf_environment& e) {
  if (e.flags & ~(SDF_ENV_SKY | SDF_ENV_SUN | SDF_ENV_FOG)) return SDF_E_INVALID_ARG;
  if ((e.flags & SDF_ENV_SUN) && !(e.flags & SDF_ENV_SKY)) return SDF_E_INVALID_ARG;
  if (e.flags & SDF_ENV_SKY)
    if (!finite3(e.horizon) || !finite3(e.zenith) || !finite3(e.ground)) return SDF_E_INVALID_ARG;
  if (e.flags & SDF_ENV_SUN)
    if (!finite3(e.sun_dir) || !finite3(e.sun_color) || !std::isfinite(e.sun_exponent) ||
        !(e.sun_exponent >= 1.0f))
      return SDF_E_INVALID_ARG;
  if (e.flags & SDF_ENV_FOG) {
    if (!finite3(e.fog_color) || !std::isfinite(e.fog_start) || !std::isfinite(e.fog_end))
      return SDF_E_INVALID_ARG;
    // the kernels divide by den (exact) or multiply by RN(1 / den) (fast):
    // both must be numbers above 0
    const float den = e.fog_end - e.fog_start;   // RN: this unit never contracts
    if (!(den > 0.0f) || !std::isfinite(den) || !std::isfinite(1.0f / den))
      return SDF_E_INVALID_ARG;
  }
  return SDF_OK;
}

// every entry's amb, dif and ref are materials[0]'s byte for byte (the three
// lead the struct; the shininess apart): the frame has one material
bool one_material(const sdf_material* materials, int32_t n) {
  for (int i = 1; i < n; ++i)
    if (std::memcmp(&materials[i], &materials[0], offsetof(sdf_material, shininess)) != 0)
      return false;
  return true;
}
// the call is sdf_render_materials itself: no bounce, and the composite or
// layer 0's colour asked for
bool reflect_is_materials(const sdf_reflect& r) {
  return r.bounces == 0 && !(r.flags & SDF_REFLECT_WEIGHT);
}

bool no_device() {
  int ndev = 0;
  return hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0;
}

}  // namespace

namespace sdf {

int validate_camera(const sdf_camera* camera) {
  if (!camera) return SDF_E_INVALID_ARG;
  for (float v : camera->view)
    if (!std::isfinite(v)) return SDF_E_INVALID_ARG;
  if (!std::isfinite(camera->fov_deg) || !std::isfinite(camera->pi)) return SDF_E_INVALID_ARG;
  for (float v : camera->eye)
    if (!(std::fabs(v) <= kMaxCoord)) return SDF_E_INVALID_ARG;
  float inv[16];
  if (!invert_view(camera->view, inv)) return SDF_E_INVALID_ARG;
  for (float v : inv)
    if (!(std::fabs(v) <= kMaxCoord)) return SDF_E_INVALID_ARG;
  // the hoisted camera position inverse(V_mat) * (eye, 1) (voxel_fragment.frag:180)
  for (int i = 0; i < 3; ++i) {
    const double c = (double)inv[i] * camera->eye[0] + (double)inv[4 + i] * camera->eye[1] +
                     (double)inv[8 + i] * camera->eye[2] + inv[12 + i];
    if (!(std::fabs(c) <= kMaxCoord)) return SDF_E_INVALID_ARG;
  }
  return SDF_OK;
}

// The order matters where SDF_E_UNSUPPORTED competes with SDF_E_INVALID_ARG.
int validate_request(const Request& r, Depth depth, bool framed) {
  const bool env = depth >= kEnv && r.env && r.env->flags != 0;
  int rc = env ? validate_environment(*r.env) : SDF_OK;
  if (rc == SDF_OK && depth >= kReflect) rc = validate_reflect(r.reflect);
  if (rc != SDF_OK) return rc;
  if (depth >= kMaterials) {
    if (!r.materials || !r.scene) return SDF_E_INVALID_ARG;
    // one material per primitive; a Mandelbulb has one
    const int32_t want = r.scene->kind == SDF_SCENE_PRIMITIVES ? r.scene->count : 1;
    if (r.nmaterials < 1 || r.nmaterials > SDF_MAX_PRIMS || r.nmaterials != want)
      return SDF_E_INVALID_ARG;
  }
  rc = validate_lights(r.lights, r.nlights, r.light_flags);
  if (rc != SDF_OK) return rc;
  // a material's checks are its presence alone
  if (!r.scene || !r.materials || !r.params) return SDF_E_INVALID_ARG;
  rc = validate_params(*r.params, r.tiling);
  if (rc == SDF_OK) rc = validate_scene(*r.scene);
  if (rc == SDF_OK && framed) rc = validate_camera(r.camera);
  if (rc != SDF_OK) return rc;
  // valid requests no kernel serves: shading terms do not average to the
  // colour, so no stream is resolved from sub-samples, and a stream carries
  // one light's and one material's terms of one layer, and no sky or fog
  const bool stream = is_stream(r.params->output_format);
  if (r.params->samples > 1 && stream) return SDF_E_UNSUPPORTED;
  if ((r.nlights > 1 || r.light_flags != 0) && stream) return SDF_E_UNSUPPORTED;
  if (depth >= kMaterials) {
    // the exponent is frame-wide: the bits of materials[0].shininess everywhere
    for (int i = 1; i < r.nmaterials; ++i)
      if (std::memcmp(&r.materials[i].shininess, &r.materials[0].shininess, sizeof(float)) != 0)
        return SDF_E_UNSUPPORTED;
    if (!one_material(r.materials, r.nmaterials) && stream) return SDF_E_UNSUPPORTED;
  }
  if (depth >= kReflect) {
    // a reflected layer's colour feeds the next weight and the composite: the
    // components must be numbers
    if (r.reflect->bounces >= 1)
      for (int i = 0; i < r.nmaterials; ++i)
        if (!finite3(r.materials[i].amb) || !finite3(r.materials[i].dif) ||
            !finite3(r.materials[i].ref))
          return SDF_E_INVALID_ARG;
    if (!reflect_is_materials(*r.reflect) && stream) return SDF_E_UNSUPPORTED;
  }
  return env && stream ? SDF_E_UNSUPPORTED : SDF_OK;
}

// The kernel family a validated request needs: the collapse rules.  A request
// that collapses takes the lower family's path, kernels and bits.
static Depth route(const Request& r) {
  if (r.env && r.env->flags != 0) return kEnv;
  if (r.reflect && !reflect_is_materials(*r.reflect)) return kReflect;
  if (!one_material(r.materials, r.nmaterials)) return kMaterials;   // a Mandelbulb: never
  return r.nlights == 1 && r.light_flags == 0 ? kPlain : kLights;
}

void plan_set_camera(RenderPlan* plan, const sdf_camera* camera) {
  KernelArgs& a = plan->a;
  invert_view(camera->view, a.inv_view);
  const float* m = a.inv_view;
  // :180 camera.pos = (inverse(V_mat) * vec4(camera.pos, 1)).xyz, fp32
  for (int i = 0; i < 3; ++i)
    a.cam[i] = m[i] * camera->eye[0] + m[4 + i] * camera->eye[1] + m[8 + i] * camera->eye[2] +
               m[12 + i] * 1.0f;
  // :191 -2.0f / tan(camera.fov * PI / 360.0f), fp32
  const float ang = camera->fov_deg * camera->pi / 360.0f;
  a.focal = -2.0f / tanf(ang);
  a.aspect = camera->aspect > 0.0f ? camera->aspect : (float)a.width / (float)a.height;
}

// The pixel grid of a width x height frame and the camera behind it.
static void plan_view(RenderPlan* plan, const sdf_camera& camera, int width, int height) {
  KernelArgs& a = plan->a;
  a.width = width;
  a.height = height;
  a.inv_width = 1.0f / (float)width;
  a.inv_height = 1.0f / (float)height;
  plan_set_camera(plan, &camera);
}

// The frame step of a validated request's plan, on a zeroed plan: the rows,
// the camera, the tiling's geometry, the outputs and the size of a TILES stream.
// With plan->rows = 0 nothing is to be rendered (SDF_OK).
static int plan_frame(const sdf_camera& camera, const sdf_params& params, const sdf_tiling* tiling,
                      void* rgba, int32_t* steps, RenderPlan* plan) {
  // Supersampling (params.samples = S > 1): the kernel is handed the S W x
  // S H sub-sample frame, whose pixel grid is exactly the request's S x S
  // sub-sample grid ((2x+1)/W - 1 at S W), under the request's tiling with
  // block_rows S times as long: S times the rows, every block and the frame's
  // last row a multiple of S.  The plan's rows (what a schedule matches and
  // the grid covers) are sub-sample rows.
  const int S = params.samples > 1 ? params.samples : 1;
  sdf_tiling t = tiling ? *tiling : kWholeFrame;
  t.block_rows *= S;
  const int rows = count_rows(params.height * S, t);
  plan->rows = rows;
  if (rows == 0) return SDF_OK;  // a rank that owns no block: nothing to write
  if (!rgba) return SDF_E_INVALID_ARG;
  if (no_device()) return SDF_E_NO_DEVICE;

  KernelArgs& a = plan->a;
  plan_view(plan, camera, params.width * S, params.height * S);
  a.out_width = params.width;
  a.ss_log2 = S == 4 ? 2 : S == 2 ? 1 : 0;
  a.block_rows = t.block_rows;
  a.chunk_rows = t.block_rows * sdf::tiling_run(t);
  a.run_gap_rows = sdf::tiling_gap_rows(t);
  a.first_block = t.first_block;
  a.block_stride = t.block_stride;
  a.rows = rows;
  a.frame_rows = (t.flags & SDF_TILING_FRAME_ROWS) ? 1 : 0;
  a.rgba = rgba;
  a.steps = steps;
  plan->tiles_ntiles = params.output_format == SDF_FORMAT_TILES
                           ? ((params.width + 7) / 8) * ((rows + 7) / 8)
                           : 0;
  // TILES offsets and the `used` header word are uint32 (tiles.hip): a
  // stream whose worst case would not fit them is refused, not wrapped
  if (plan->tiles_ntiles > 0 && TilesLayout(plan->tiles_ntiles).stream_end > 0xffffffffull)
    return SDF_E_UNSUPPORTED;
  return SDF_OK;
}

// The scene step: the primitive blocks and the culling bounds, the march and
// shading parameters under one light and one material, and the kernel that
// serves the scene (variant, precision, JIT flag and signature).
static void plan_scene(const sdf_scene& scene, const sdf_light& light,
                       const sdf_material& material, const sdf_params& params, RenderPlan* plan) {
  KernelArgs& a = plan->a;
  for (int i = 0; i < 3; ++i) {
    a.light_pos[i] = light.pos[i];
    a.mat_amb[i] = material.amb[i];
    a.mat_dif[i] = material.dif[i];
    a.mat_ref[i] = material.ref[i];
  }
  a.light_amb = light.ambient;
  a.shininess = material.shininess;
  a.max_steps = params.max_steps;
  a.max_dist = params.max_dist;
  a.eps = params.eps;
  a.shadow_k = params.shadow_k;
  a.normal_eps = params.normal_eps;
  a.shadow_offset = params.shadow_offset;
  a.flags = params.flags;
  a.normal_mode = params.normal_mode;
  a.format = params.output_format;
  a.ao_taps = (params.flags & SDF_FLAG_AO) ? params.ao_taps : 0;
  a.ao_step = params.ao_step;
  a.ao_base = params.ao_base;
  a.ao_falloff = params.ao_falloff;
  a.ao_strength = params.ao_strength;
  // AO tap heights, in the oracle's fp32 operation order (oracle_core.h
  // ambient_occlusion): t = i / (taps - 1); h = base + step * t
  for (int i = 0; i < a.ao_taps && i < kMaxAoTaps; ++i) {
    const float tt = a.ao_taps > 1 ? (float)i / (float)(a.ao_taps - 1) : 0.0f;
    a.ao_h[i] = params.ao_base + params.ao_step * tt;
  }
  // the AO taps' path lengths from P, visited in order (trace.inc trace_shape):
  // |h_0| + sum |h_k - h_(k-1)|, rounded up to fp32 so it never undercounts
  {
    double path = 0.0;
    for (int i = 0; i < a.ao_taps && i < kMaxAoTaps; ++i) {
      path += std::fabs((double)a.ao_h[i] - (i ? (double)a.ao_h[i - 1] : 0.0));
      float f = (float)path;
      if ((double)f < path) f = std::nextafter(f, INFINITY);
      a.ao_path[i] = f;
    }
  }
  a.scene_kind = scene.kind;
  a.prim_count = scene.kind == SDF_SCENE_PRIMITIVES ? scene.count : 0;
  for (int i = 0; i < 3; ++i) a.bulb_center[i] = scene.bulb_center[i];
  a.bulb_scale = scene.bulb_scale;
  a.bulb_bail2 = scene.bulb_bailout * scene.bulb_bailout;
  a.bulb_iterations = scene.bulb_iterations;
  a.bulb_inv_scale = 1.0f / scene.bulb_scale;
  prepare_prims(scene, a.prims);
  // the generic kernel on request, and beyond the culling's proven range
  // (there unculled); only the specialised kernels carry gaps along a path
  const bool prims = scene.kind == SDF_SCENE_PRIMITIVES;
  const bool exact = params.precision == SDF_PRECISION_EXACT;
  const bool cached = params.dispatch == SDF_DISPATCH_AUTO;
  const bool cull_proven = !prims || prepare_bounds(scene, a, exact, cached, params.max_dist);
  const bool generic = (!cached || !cull_proven) && prims;
  if (params.dispatch == SDF_DISPATCH_UNCULLED || !cull_proven) a.cluster_first = a.prim_count;
  plan->variant = generic ? kVariantGeneric : select_variant(scene);
  plan->exact = exact;
  // no built-in specialisation: a run-time compiled one (jit.cpp)
  plan->jit = plan->variant == kVariantGeneric && !generic && a.prim_count > 0;
  if (plan->jit) plan->nsig = scene_signature(scene, plan->sig);
}

// Both steps for a validated request under its first light and material.
static int plan_request(const Request& r, void* rgba, int32_t* steps, RenderPlan* plan) {
  std::memset(plan, 0, sizeof(*plan));
  const int rc = plan_frame(*r.camera, *r.params, r.tiling, rgba, steps, plan);
  if (rc == SDF_OK && plan->rows > 0)
    plan_scene(*r.scene, r.lights[0], r.materials[0], *r.params, plan);
  return rc;
}

int make_render_plan(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* light,
                     const sdf_material* material, const sdf_params* params,
                     const sdf_tiling* tiling, void* rgba, int32_t* steps, RenderPlan* plan) {
  const Request r = {scene, camera, light, 1, 0, material, 1, nullptr, nullptr, params, tiling};
  const int rc = validate_request(r, kPlain);
  if (rc != SDF_OK) return rc;
  if (!plan) return SDF_E_INVALID_ARG;
  return plan_request(r, rgba, steps, plan);
}

int launch_render_plan(const RenderPlan& plan, void* stream) {
  if (plan.rows == 0) return SDF_OK;
  RenderArgs r;
  r.a = plan.a;
  r.o.cost = plan.order.cost;
  r.o.n = plan.order.n;
  r.o.reserved = 0;
  std::memcpy(r.o.order, plan.order.order, sizeof(uint16_t) * (size_t)std::max(plan.order.n, 0));
  r.l = plan.lights;
  r.m = plan.materials;
  r.r = plan.reflect;
  r.e = plan.env;
  const int rc = launch_planned(plan, launch_render_jit, &RenderUnit::render, r, stream);
  if (rc != SDF_OK || plan.tiles_ntiles == 0) return rc;
  const int err = launch_tiles_compact(plan.a.rgba, plan.tiles_ntiles, stream, plan.tiles_used);
  return err == hipSuccess ? SDF_OK : SDF_E_HIP;
}

// ---- render schedules (sdf_schedule) ---------------------------------------
// The kernels add each wave's shader-clock cycles to its 8-row block's cost
// word (RowOrder::cost).  Every `period` launches the schedule copies the
// words to pinned host memory behind the launch; once such a copy has landed
// (an event query: the host never waits), the cost of every block since the
// previous snapshot orders the blocks for the next launches, costliest first
// (LPT order: a frame's longest tiles start first, and short ones fill the
// end of the frame instead of the longest ones running alone).  The order is
// a permutation by construction and rides in the kernel arguments, so the
// measurement is a heuristic only: every block is rendered exactly once
// whatever the costs say.
struct Schedule {
  int rows = 0, nblocks = 0, period = 1;
  int dev = 0;
  unsigned long long* cost = nullptr;   // device, nblocks words (accumulating)
  unsigned long long* snap = nullptr;   // pinned host, nblocks words
  std::vector<unsigned long long> last; // the previous snapshot
  hipEvent_t ev = nullptr;
  bool pending = false;
  bool measure = false;                 // the launch being prepared measures its costs
  long long launches = 0;
  int n = 0;                            // 0 until the first order is known
  std::vector<uint16_t> order;
};

Schedule* schedule_create(int rows, int period) {
  auto* s = new Schedule();
  s->rows = rows;
  s->nblocks = (rows + 7) / 8;
  s->period = period > 0 ? period : 1;
  s->last.assign(s->nblocks, 0ull);
  s->order.resize(s->nblocks);
  bool ok = hipGetDevice(&s->dev) == hipSuccess && s->nblocks <= kMaxOrderBlocks;
  const size_t bytes = sizeof(unsigned long long) * std::max(s->nblocks, 1);
  ok = ok && hipMalloc((void**)&s->cost, bytes) == hipSuccess &&
       hipMemset(s->cost, 0, bytes) == hipSuccess &&
       hipHostMalloc((void**)&s->snap, bytes, hipHostMallocDefault) == hipSuccess &&
       hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) == hipSuccess &&
       hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    schedule_destroy(s);
    return nullptr;
  }
  return s;
}

void schedule_destroy(Schedule* s) {
  if (!s) return;
  if (s->ev) {
    (void)hipEventSynchronize(s->ev);
    (void)hipEventDestroy(s->ev);
  }
  if (s->cost) (void)hipFree(s->cost);
  if (s->snap) (void)hipHostFree(s->snap);
  delete s;
}

int schedule_apply(Schedule* s, RenderPlan* plan) {
  plan->order.n = 0;
  plan->order.cost = nullptr;
  if (!s || plan->rows != s->rows) return SDF_OK;   // another shape: launch order, no costs
  const hipError_t q = s->pending ? hipEventQuery(s->ev) : hipErrorNotReady;
  if (s->pending && q != hipSuccess && q != hipErrorNotReady) {
    // the copy of the costs failed: stop waiting for it and
    // report the error; the next call measures again
    (void)hipGetLastError();
    s->pending = false;
    return SDF_E_HIP;
  }
  if (s->pending && q == hipSuccess) {
    s->pending = false;
    std::vector<std::pair<unsigned long long, int>> d(s->nblocks);
    unsigned long long total = 0;
    for (int b = 0; b < s->nblocks; ++b) {
      const unsigned long long v = s->snap[b] - s->last[b];
      s->last[b] = s->snap[b];
      d[b] = {v, b};
      total += v;
    }
    if (total > 0) {
      // costliest first; ties (and blocks not measured) in launch order
      std::stable_sort(d.begin(), d.end(), [](const auto& x, const auto& y) {
        return x.first > y.first;
      });
      for (int i = 0; i < s->nblocks; ++i) s->order[i] = (uint16_t)d[i].second;
      s->n = s->nblocks;
    }
  }
  // only the launch whose costs are copied out measures them (every wave's
  // clock reads and its atomic add cost the others nothing)
  s->measure = !s->pending && (s->launches % s->period) == 0;
  plan->order.cost = s->measure ? s->cost : nullptr;
  plan->order.n = s->n;
  if (s->n) std::memcpy(plan->order.order, s->order.data(), sizeof(uint16_t) * s->n);
  return SDF_OK;
}

int schedule_after(Schedule* s, void* stream) {
  if (!s) return SDF_OK;
  s->launches++;
  if (!s->measure) return SDF_OK;
  s->measure = false;
  if (hipMemcpyAsync(s->snap, s->cost, sizeof(unsigned long long) * s->nblocks,
                     hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipEventRecord(s->ev, (hipStream_t)stream) != hipSuccess)
    return SDF_E_HIP;
  s->pending = true;
  return SDF_OK;
}

}  // namespace sdf

struct sdf_schedule {
  sdf::Schedule* s;
};

// The launch of a made plan under `schedule` (null: launch order, no costs):
// the schedule's order and cost words into the plan, the launch, and the
// schedule's bookkeeping when the plan has the schedule's rows.
static int run_plan(sdf::RenderPlan& plan, sdf_schedule* schedule, void* stream) {
  if (!schedule) return sdf::launch_render_plan(plan, stream);
  int rc = sdf::schedule_apply(schedule->s, &plan);
  if (rc != SDF_OK) return rc;
  rc = sdf::launch_render_plan(plan, stream);
  if (rc == SDF_OK && plan.rows == schedule->s->rows)
    rc = sdf::schedule_after(schedule->s, stream);
  return rc;
}

// The launch's lights (sdf_render_lights).  The lights kernels serve every
// L >= 1, one plain light included.
static void fill_lights(sdf::RenderPlan& plan, const sdf_light* lights, int32_t n, int32_t flags) {
  sdf::LightsArgs& l = plan.lights;
  l.n = n;
  l.flags = flags;
  // the summed ambient: fp32, index order (this unit is built without
  // contraction; one light gives its own value)
  float la = lights[0].ambient;
  for (int i = 1; i < n; ++i) la = la + lights[i].ambient;
  l.la = la;
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) {
      l.pos[i][c] = lights[i].pos[c];
      l.color[i][c] = lights[i].color[c];
    }
}

// The launch's material table, one row per primitive (sdf_render_materials).
static void fill_materials(sdf::RenderPlan& plan, const sdf_material* materials, int32_t n) {
  sdf::MaterialArgs& m = plan.materials;
  m.n = n;
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) {
      m.m[i][c] = materials[i].amb[c];
      m.m[i][3 + c] = materials[i].dif[c];
      m.m[i][6 + c] = materials[i].ref[c];
    }
}

// A validated environment's uniforms (flags != 0): the fields of the features
// that are on; the rest stays zero
static sdf::EnvArgs fill_env(const sdf_environment& env) {
  sdf::EnvArgs e{};
  e.on = 1;
  e.flags = env.flags;
  if (env.flags & SDF_ENV_SKY)
    for (int c = 0; c < 3; ++c) {
      e.horizon[c] = env.horizon[c];
      e.zenith[c] = env.zenith[c];
      e.ground[c] = env.ground[c];
    }
  if (env.flags & SDF_ENV_SUN) {
    for (int c = 0; c < 3; ++c) {
      e.sun_dir[c] = env.sun_dir[c];
      e.sun_color[c] = env.sun_color[c];
    }
    e.sun_exponent = env.sun_exponent;
  }
  if (env.flags & SDF_ENV_FOG) {
    for (int c = 0; c < 3; ++c) e.fog_color[c] = env.fog_color[c];
    e.fog_end = env.fog_end;
    e.fog_den = env.fog_end - env.fog_start;   // RN, > 0 (validate_environment)
    e.fog_inv = 1.0f / e.fog_den;
  }
  return e;
}

// What the kernels of `family` read beside the plan's one light and material,
// from a validated request.  Every family above kPlain is a lights kernel (for
// every L >= 1, one plain light included); the reflect and env kernels fold
// the table of every primitive scene (a Mandelbulb's one material is the
// plan's own).
static void fill_plan(sdf::RenderPlan& plan, const sdf::Request& r, sdf::Depth family) {
  if (family >= sdf::kLights) fill_lights(plan, r.lights, r.nlights, r.light_flags);
  if (family >= sdf::kMaterials && r.scene->kind == SDF_SCENE_PRIMITIVES)
    fill_materials(plan, r.materials, r.nmaterials);
  if (family >= sdf::kReflect)   // on, bounces, strength, layer, weight
    plan.reflect = {1, r.reflect->bounces, r.reflect->strength, r.reflect->layer,
                    (r.reflect->flags & SDF_REFLECT_WEIGHT) ? 1 : 0, {0, 0, 0}};
  if (family >= sdf::kEnv) plan.env = fill_env(*r.env);
}

// Every frame render: the request validated once at the entry point's depth,
// routed to its kernel family, planned and launched.
static int render_request(const sdf::Request& r, sdf::Depth depth, void* rgba, int32_t* steps,
                          sdf_schedule* schedule, void* stream) {
  int rc = sdf::validate_request(r, depth);
  if (rc != SDF_OK) return rc;
  sdf::RenderPlan plan;
  rc = sdf::plan_request(r, rgba, steps, &plan);
  if (rc != SDF_OK) return rc;
  fill_plan(plan, r, sdf::route(r));
  return run_plan(plan, schedule, stream);
}

extern "C" {

int sdf_abi_version(void) { return SDF_ABI_VERSION; }

int sdf_schedule_create(int32_t rows, int32_t period, sdf_schedule** out) {
  if (!out) return SDF_E_INVALID_ARG;
  *out = nullptr;
  if (rows <= 0 || rows > 8 * sdf::kMaxOrderBlocks || period < 1) return SDF_E_INVALID_ARG;
  sdf::Schedule* s = sdf::schedule_create(rows, period);
  if (!s) return SDF_E_HIP;
  *out = new sdf_schedule{s};
  return SDF_OK;
}

int sdf_schedule_destroy(sdf_schedule* s) {
  if (!s) return SDF_OK;
  sdf::schedule_destroy(s->s);
  delete s;
  return SDF_OK;
}

int sdf_schedule_order(const sdf_schedule* s, int32_t* order, int32_t n) {
  if (!s || (n > 0 && !order)) return SDF_E_INVALID_ARG;
  for (int i = 0; i < n && i < s->s->n; ++i) order[i] = s->s->order[i];
  return s->s->n;
}

int sdf_render_scheduled(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* light,
                         const sdf_material* material, const sdf_params* params,
                         const sdf_tiling* tiling, void* rgba, int32_t* steps,
                         sdf_schedule* schedule, void* stream) {
  return render_request({scene, camera, light, 1, 0, material, 1, nullptr, nullptr, params, tiling},
                        sdf::kPlain, rgba, steps, schedule, stream);
}

int sdf_defaults(sdf_scene* scene, sdf_camera* camera, sdf_light* light,
                 sdf_material* material, sdf_params* params, int32_t width, int32_t height) {
  if (scene) {
    std::memset(scene, 0, sizeof(*scene));
    scene->kind = SDF_SCENE_PRIMITIVES;
    scene->count = 2;
    // sceneSDF (voxel_fragment.frag:73-81): min(min(INF, planeSDF), sphereSDF)
    sdf_primitive& plane = scene->prims[0];   // planeSDF :66-71 -> p.y
    plane.kind = SDF_PRIM_PLANE;
    plane.op = SDF_OP_UNION;
    plane.p[1] = 1.0f;
    sdf_primitive& sphere = scene->prims[1];  // sphereSDF :54-64
    sphere.kind = SDF_PRIM_SPHERE;
    sphere.op = SDF_OP_UNION;
    sphere.p[1] = 0.4f;
    sphere.p[3] = 0.2f;
    scene->bulb_scale = 1.0f;
    scene->bulb_iterations = 12;
    scene->bulb_bailout = 2.0f;
  }
  if (camera) {
    std::memset(camera, 0, sizeof(*camera));
    for (int i = 0; i < 4; ++i) camera->view[i * 5] = 1.0f;  // orbit/pan 0 (main.cpp:7-11)
    camera->eye[1] = 0.2f;                                     // :179
    camera->eye[2] = 2.0f;
    camera->fov_deg = 60.0f;                                   // :178
    camera->aspect = 0.0f;                                     // AR = W / H
    camera->pi = 3.1415925359f;                                // :15 (sic)
  }
  if (light) {
    std::memset(light, 0, sizeof(*light));
    light->pos[0] = 5.0f;                                      // :182
    light->pos[1] = 5.0f;
    light->ambient = 0.1f;                                     // :184
    light->color[0] = light->color[1] = light->color[2] = 0.7f; // :183 (unused)
  }
  if (material) {
    std::memset(material, 0, sizeof(*material));
    material->amb[1] = 0.2f;                                   // :186
    material->amb[2] = 0.8f;
    material->dif[1] = 0.2f;                                   // :187
    material->dif[2] = 0.8f;
    material->ref[0] = material->ref[1] = material->ref[2] = 0.5f; // :188
    material->shininess = 12.0f;                               // :189
  }
  if (params) {
    std::memset(params, 0, sizeof(*params));
    params->width = width > 0 ? width : 800;                   // main.cpp:4
    params->height = height > 0 ? height : 600;                // main.cpp:5
    params->max_steps = 100;                                   // :17
    params->max_dist = 100.0f;                                 // :18
    params->eps = 0.01f;                                       // :19
    params->shadow_k = 10.0f;                                  // :205
    params->normal_eps = 0.01f;                                // :21-23
    params->shadow_offset = 2.0f;                              // :205
    params->flags = SDF_FLAG_SHADOW;
    params->normal_mode = SDF_NORMAL_CENTRAL;
    params->ao_taps = 5;
    params->ao_step = 0.12f;
    params->ao_base = 0.01f;
    params->ao_falloff = 0.95f;
    params->ao_strength = 3.0f;
    params->precision = SDF_PRECISION_EXACT;
  }
  return SDF_OK;
}

int sdf_share_tiling(int32_t rank, int32_t world, int32_t share_root, int32_t share_peer,
                     sdf_tiling* tiling) {
  if (!tiling || world < 1 || rank < 0 || rank >= world || share_root < 1 || share_peer < 1)
    return SDF_E_INVALID_ARG;
  const int a = share_root, b = share_peer;
  if (world == 1) {
    *tiling = kWholeFrame;
  } else {
    // peers' blocks interleave (world - 1 apart), so the frame's last partial
    // period spreads over distinct ranks instead of one peer's whole run
    *tiling = sdf_tiling{8, rank == 0 ? 0 : a + rank - 1, a + b * (world - 1), 0,
                         rank == 0 ? a : b, rank == 0 || b == 1 ? 1 : world - 1};
  }
  return SDF_OK;
}

int sdf_owned_rows(int32_t height, const sdf_tiling* tiling) {
  return count_rows(height, tiling ? *tiling : kWholeFrame);
}

int sdf_validate(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* light,
                 const sdf_material* material, const sdf_params* params,
                 const sdf_tiling* tiling) {
  return sdf::validate_request(
      {scene, camera, light, 1, 0, material, 1, nullptr, nullptr, params, tiling}, sdf::kPlain);
}

int sdf_format_bytes(int32_t format) {
  switch (format) {
    case SDF_FORMAT_RGBA32F: return 16;
    case SDF_FORMAT_RGBA16F: return 8;
    case SDF_FORMAT_RGBA8: return 4;
    case SDF_FORMAT_RGB32F: return 12;
    case SDF_FORMAT_TILES: return SDF_E_UNSUPPORTED;   // size is per stream
    case SDF_FORMAT_SHADE32F: return 16;
    default: return SDF_E_INVALID_ARG;
  }
}

// TILES buffer: the stream (header, offset table, worst-case records of 3 x
// 32 bit planes) and the encoder's scratch (kernel_args.h TilesLayout)
int64_t sdf_tiles_bytes(int32_t width, int32_t rows) {
  if (width <= 0 || rows < 0) return SDF_E_INVALID_ARG;
  const int64_t ntiles = int64_t((width + 7) / 8) * ((rows + 7) / 8);
  if (sdf::TilesLayout(ntiles).stream_end > 0xffffffffull) return SDF_E_UNSUPPORTED;
  return (int64_t)sdf::TilesLayout(ntiles).end;
}

int sdf_render(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* light,
               const sdf_material* material, const sdf_params* params,
               const sdf_tiling* tiling, void* rgba, int32_t* steps, void* stream) {
  return render_request({scene, camera, light, 1, 0, material, 1, nullptr, nullptr, params, tiling},
                        sdf::kPlain, rgba, steps, nullptr, stream);
}

int sdf_validate_lights(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* lights,
                        int32_t nlights, int32_t light_flags, const sdf_material* material,
                        const sdf_params* params, const sdf_tiling* tiling) {
  return sdf::validate_request({scene, camera, lights, nlights, light_flags, material, 1, nullptr,
                                nullptr, params, tiling}, sdf::kLights);
}

int sdf_render_lights(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* lights,
                      int32_t nlights, int32_t light_flags, const sdf_material* material,
                      const sdf_params* params, const sdf_tiling* tiling, void* rgba,
                      int32_t* steps, sdf_schedule* schedule, void* stream) {
  return render_request({scene, camera, lights, nlights, light_flags, material, 1, nullptr,
                         nullptr, params, tiling},
                        sdf::kLights, rgba, steps, schedule, stream);
}

int sdf_validate_materials(const sdf_scene* scene, const sdf_camera* camera,
                           const sdf_light* lights, int32_t nlights, int32_t light_flags,
                           const sdf_material* materials, int32_t nmaterials,
                           const sdf_params* params, const sdf_tiling* tiling) {
  return sdf::validate_request({scene, camera, lights, nlights, light_flags, materials, nmaterials,
                                nullptr, nullptr, params, tiling}, sdf::kMaterials);
}

int sdf_render_materials(const sdf_scene* scene, const sdf_camera* camera,
                         const sdf_light* lights, int32_t nlights, int32_t light_flags,
                         const sdf_material* materials, int32_t nmaterials,
                         const sdf_params* params, const sdf_tiling* tiling, void* rgba,
                         int32_t* steps, sdf_schedule* schedule, void* stream) {
  return render_request({scene, camera, lights, nlights, light_flags, materials, nmaterials,
                         nullptr, nullptr, params, tiling},
                        sdf::kMaterials, rgba, steps, schedule, stream);
}

int sdf_validate_reflect(const sdf_scene* scene, const sdf_camera* camera,
                         const sdf_light* lights, int32_t nlights, int32_t light_flags,
                         const sdf_material* materials, int32_t nmaterials,
                         const sdf_reflect* reflect, const sdf_params* params,
                         const sdf_tiling* tiling) {
  return sdf::validate_request({scene, camera, lights, nlights, light_flags, materials, nmaterials,
                                reflect, nullptr, params, tiling}, sdf::kReflect);
}

int sdf_render_reflect(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* lights,
                       int32_t nlights, int32_t light_flags, const sdf_material* materials,
                       int32_t nmaterials, const sdf_reflect* reflect, const sdf_params* params,
                       const sdf_tiling* tiling, void* rgba, int32_t* steps,
                       sdf_schedule* schedule, void* stream) {
  return render_request({scene, camera, lights, nlights, light_flags, materials, nmaterials,
                         reflect, nullptr, params, tiling},
                        sdf::kReflect, rgba, steps, schedule, stream);
}

int sdf_validate_env(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* lights,
                     int32_t nlights, int32_t light_flags, const sdf_material* materials,
                     int32_t nmaterials, const sdf_reflect* reflect, const sdf_environment* env,
                     const sdf_params* params, const sdf_tiling* tiling) {
  return sdf::validate_request({scene, camera, lights, nlights, light_flags, materials, nmaterials,
                                reflect, env, params, tiling}, sdf::kEnv);
}

int sdf_render_env(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* lights,
                   int32_t nlights, int32_t light_flags, const sdf_material* materials,
                   int32_t nmaterials, const sdf_reflect* reflect, const sdf_environment* env,
                   const sdf_params* params, const sdf_tiling* tiling, void* rgba, int32_t* steps,
                   sdf_schedule* schedule, void* stream) {
  return render_request({scene, camera, lights, nlights, light_flags, materials, nmaterials,
                         reflect, env, params, tiling},
                        sdf::kEnv, rgba, steps, schedule, stream);
}

// ---- queries (sdf_abi.h "Queries") ------------------------------------------
namespace {
constexpr int64_t kMaxQuery = int64_t(1) << 30;

// The params a query is validated and run with: the fields it uses taken from
// the caller's, every other one at sdf_defaults' value (`frame`: the camera
// form also uses width and height).
sdf_params query_params(const sdf_params& p, bool frame) {
  sdf_params q;
  sdf_defaults(nullptr, nullptr, nullptr, nullptr, &q, 0, 0);
  if (frame) {
    q.width = p.width;
    q.height = p.height;
  }
  q.max_steps = p.max_steps;
  q.max_dist = p.max_dist;
  q.eps = p.eps;
  q.normal_eps = p.normal_eps;
  q.normal_mode = p.normal_mode;
  q.precision = p.precision;
  q.dispatch = p.dispatch;
  return q;
}

// a query's own checks: its params, its scene, and its camera where it has one
int validate_query(const sdf_scene* scene, const sdf_camera* camera, const sdf_params& q) {
  int rc = validate_params(q, nullptr);
  if (rc == SDF_OK && scene) rc = validate_scene(*scene);
  if (rc == SDF_OK && camera) rc = sdf::validate_camera(camera);
  return rc;
}

// The prepared scene of a validated call that renders no frame (a query, a
// mesh, a gradient, rays, points), under the call's params `q`: the plan's
// scene step alone, and the pixel grid of `camera` where the call has one.  No
// outputs.  `light`, `material`: the call's own where it shades; sdf_defaults'
// otherwise, which the kernel arguments then carry.
int scene_plan(const sdf_scene* scene, const sdf_camera* camera, const sdf_params& q,
               sdf::RenderPlan* plan, const sdf_light* light = nullptr,
               const sdf_material* material = nullptr) {
  if (no_device()) return SDF_E_NO_DEVICE;
  sdf_light l;
  sdf_material m;
  if (!light || !material) sdf_defaults(nullptr, nullptr, &l, &m, nullptr, 0, 0);
  std::memset(plan, 0, sizeof(*plan));
  if (camera) sdf::plan_view(plan, *camera, q.width, q.height);
  sdf::plan_scene(*scene, light ? *light : l, material ? *material : m, q, plan);
  return SDF_OK;
}

// One validated query: the scene's plan with the query's buffers.
int query_launch(int kind, const sdf_scene* scene, const sdf_camera* camera, const sdf_params& q,
                 const float* in0, const float* in1, int64_t n, float* t, int32_t* steps,
                 float* normal, int32_t* prim, void* stream) {
  std::unique_ptr<sdf::RenderPlan> plan(new sdf::RenderPlan());
  const int rc = scene_plan(scene, camera, q, plan.get());
  if (rc != SDF_OK) return rc;
  std::unique_ptr<sdf::QueryArgs> a(new sdf::QueryArgs());
  a->a = plan->a;
  a->in0 = in0;
  a->in1 = in1;
  a->t = t;
  a->steps = steps;
  a->normal = normal;
  a->prim = prim;
  a->n = n;
  a->kind = kind;
  a->reserved = 0;
  return sdf::launch_planned(*plan, sdf::launch_query_jit, &sdf::RenderUnit::query, *a, stream);
}
}  // namespace

int sdf_validate_query(const sdf_scene* scene, const sdf_params* params) {
  if (!scene || !params) return SDF_E_INVALID_ARG;
  return validate_query(scene, nullptr, query_params(*params, false));
}

int sdf_trace(const sdf_scene* scene, const sdf_params* params, const float* origins,
              const float* dirs, int64_t n, const sdf_hits* hits, void* stream) {
  if (!scene || !params || !hits) return SDF_E_INVALID_ARG;
  if (!hits->t && !hits->steps && !hits->normal && !hits->prim) return SDF_E_INVALID_ARG;
  if (n < 0 || n > kMaxQuery || (n > 0 && (!origins || !dirs))) return SDF_E_INVALID_ARG;
  const sdf_params q = query_params(*params, false);
  const int rc = validate_query(scene, nullptr, q);
  if (rc != SDF_OK) return rc;
  if (n == 0) return SDF_OK;   // nothing to launch, no device needed
  return query_launch(sdf::kQueryRays, scene, nullptr, q, origins, dirs, n, hits->t, hits->steps,
                      hits->normal, hits->prim, stream);
}

int sdf_trace_camera(const sdf_scene* scene, const sdf_camera* camera, const sdf_params* params,
                     const sdf_hits* hits, void* stream) {
  if (!scene || !camera || !params || !hits) return SDF_E_INVALID_ARG;
  if (!hits->t && !hits->steps && !hits->normal && !hits->prim) return SDF_E_INVALID_ARG;
  const sdf_params q = query_params(*params, true);
  const int rc = validate_query(scene, camera, q);
  if (rc != SDF_OK) return rc;
  if (params->samples > 1) return SDF_E_UNSUPPORTED;   // one ray per pixel
  return query_launch(sdf::kQueryCamera, scene, camera, q, nullptr, nullptr,
                      int64_t(q.width) * q.height, hits->t, hits->steps, hits->normal, hits->prim,
                      stream);
}

int sdf_sample(const sdf_scene* scene, const sdf_params* params, const float* points, int64_t n,
               float* dist, float* normal, void* stream) {
  if (!scene || !params) return SDF_E_INVALID_ARG;
  if (!dist && !normal) return SDF_E_INVALID_ARG;
  if (n < 0 || n > kMaxQuery || (n > 0 && !points)) return SDF_E_INVALID_ARG;
  const sdf_params q = query_params(*params, false);
  const int rc = validate_query(scene, nullptr, q);
  if (rc != SDF_OK) return rc;
  if (n == 0) return SDF_OK;
  return query_launch(sdf::kQueryPoints, scene, nullptr, q, points, nullptr, n, dist, nullptr,
                      normal, nullptr, stream);
}

// ---- isosurface meshes (sdf_abi.h "Meshes") -----------------------------------
static_assert(sizeof(sdf_grid) == 48, "sdf_grid layout");
static_assert(sizeof(sdf_mesh_out) == 48, "sdf_mesh_out layout");
static_assert(sizeof(sdf_mesh_sharp) == 16, "sdf_mesh_sharp layout");
namespace {
constexpr int64_t kMaxLattice = int64_t(1) << 30;

// The grid's own checks (no scene): sizes, finiteness, the 1e15 range, flags.
// On success *nbricks is the number of 8 x 8 x 8 bricks.
int validate_grid(const sdf_grid* g, int64_t* nbricks) {
  if (!g) return SDF_E_INVALID_ARG;
  if ((g->flags & ~SDF_MESH_DENSE) || g->reserved != 0) return SDF_E_INVALID_ARG;
  if (!(std::fabs(g->iso) <= kMaxCoord)) return SDF_E_INVALID_ARG;
  int64_t points = 1, bricks = 1;
  for (int c = 0; c < 3; ++c) {
    if (g->n[c] < 1) return SDF_E_INVALID_ARG;
    points *= int64_t(g->n[c]) + 1;   // each factor <= 2^31, checked after each product
    if (points > kMaxLattice) return SDF_E_INVALID_ARG;
    bricks *= (int64_t(g->n[c]) + 7) / 8;
    if (!(g->cell[c] > 0.0f) || !std::isfinite(g->cell[c])) return SDF_E_INVALID_ARG;
    if (!(std::fabs(g->origin[c]) <= kMaxCoord)) return SDF_E_INVALID_ARG;
    const double far = double(g->origin[c]) + double(g->n[c]) * double(g->cell[c]);
    if (!(std::fabs(far) <= kMaxCoord)) return SDF_E_INVALID_ARG;
  }
  if (nbricks) *nbricks = bricks;
  return SDF_OK;
}

int validate_mesh(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                  int64_t* nbricks) {
  if (!scene || !params || !grid) return SDF_E_INVALID_ARG;
  const int rc = validate_query(scene, nullptr, query_params(*params, false));
  if (rc != SDF_OK) return rc;
  return validate_grid(grid, nbricks);
}

// MeshArgs::skip: L R + 2^-13 V, rounded up, or +INF where the proof
// (mesh_kernel.inc) does not hold and every brick is evaluated.
float mesh_skip_bound(const sdf_scene& s, const sdf_grid& g) {
  if ((g.flags & SDF_MESH_DENSE) || s.kind != SDF_SCENE_PRIMITIVES) return INFINITY;
  double M = 0, S = 1, L = 1, diag2 = 0;
  for (int c = 0; c < 3; ++c) {
    if (int64_t(g.n[c]) + 8 >= (int64_t(1) << 24)) return INFINITY;
    const double edge = 8.0 * g.cell[c];
    const double far = double(g.origin[c]) + double(g.n[c]) * g.cell[c];
    M = std::max(M, std::max(std::fabs(double(g.origin[c])), std::fabs(far)) + edge);
    diag2 += edge * edge;
  }
  for (int i = 0; i < s.count; ++i) {
    const sdf_primitive& pr = s.prims[i];
    for (float v : pr.p) S = std::max(S, std::fabs(double(v)));
    if (smooth_op(pr.op)) S = std::max(S, double(pr.k));
    if (pr.kind == SDF_PRIM_PLANE)
      L = std::max(L, std::sqrt(double(pr.p[0]) * pr.p[0] + double(pr.p[1]) * pr.p[1] +
                                double(pr.p[2]) * pr.p[2]));
  }
  if (!(M <= 0x1p20 && S <= 0x1p20)) return INFINITY;
  const double V = 4.0 * (M + S) * S + std::fabs(double(g.iso));
  const double bound = (L * 0.5 * std::sqrt(diag2) + 0x1p-13 * V) * (1.0 + 0x1p-40);
  return std::nextafter(float(bound), INFINITY);
}

// One validated mesh call: the scene's plan with the grid and the mesh
// buffers; the count is followed by the scan that turns the bricks' counts
// into offsets and totals.
int mesh_launch(int kind, const sdf_scene* scene, const sdf_params* params, const sdf_grid* g,
                int64_t nbricks, void* workspace, int64_t* counts, const sdf_mesh_out* out,
                const sdf_mesh_sharp* sharp, void* stream) {
  const bool emit = kind != sdf::kMeshCount;
  std::unique_ptr<sdf::RenderPlan> plan(new sdf::RenderPlan());
  const int rc = scene_plan(scene, nullptr, query_params(*params, false), plan.get());
  if (rc != SDF_OK) return rc;
  std::unique_ptr<sdf::MeshArgs> m(new sdf::MeshArgs());
  m->a = plan->a;
  for (int i = 0; i < 3; ++i) {
    m->origin[i] = g->origin[i];
    m->cell[i] = g->cell[i];
    m->n[i] = g->n[i];
    m->nb[i] = (g->n[i] + 7) / 8;
  }
  m->iso = g->iso;
  m->skip = mesh_skip_bound(*scene, *g);
  m->nbricks = nbricks;
  m->ws = static_cast<unsigned char*>(workspace);
  if (emit) {
    m->verts = out->verts;
    m->tris = out->tris;
    m->normal = out->normal;
    m->prim = out->prim;
    m->max_verts = out->max_verts;
    m->max_tris = out->max_tris;
  }
  if (kind == sdf::kMeshEmitSharp) {
    m->refine = sharp->refine;
    m->iterations = sharp->iterations;
  }
  const int lrc = sdf::launch_planned(*plan, sdf::launch_mesh_jit, &sdf::RenderUnit::mesh, *m,
                                      stream, kind);
  if (lrc != SDF_OK || emit) return lrc;
  const int err = sdf::launch_mesh_scan(m->ws, nbricks, (long long*)counts, stream);
  return err == hipSuccess ? SDF_OK : SDF_E_HIP;
}

// the workspace a call was handed: present, aligned, large enough
bool mesh_workspace_fits(const void* workspace, int64_t bytes, int64_t nbricks) {
  return workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
         bytes >= (int64_t)sdf::MeshLayout(nbricks).end;
}
}  // namespace

int sdf_validate_mesh(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid) {
  return validate_mesh(scene, params, grid, nullptr);
}

int64_t sdf_mesh_workspace_bytes(const sdf_grid* grid) {
  int64_t nbricks = 0;
  const int rc = validate_grid(grid, &nbricks);
  if (rc != SDF_OK) return rc;
  return (int64_t)sdf::MeshLayout(nbricks).end;
}

int sdf_mesh_count(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                   void* workspace, int64_t workspace_bytes, int64_t* counts, void* stream) {
  int64_t nbricks = 0;
  const int rc = validate_mesh(scene, params, grid, &nbricks);
  if (rc != SDF_OK) return rc;
  if (!counts || !mesh_workspace_fits(workspace, workspace_bytes, nbricks)) return SDF_E_INVALID_ARG;
  return mesh_launch(sdf::kMeshCount, scene, params, grid, nbricks, workspace, counts, nullptr,
                     nullptr, stream);
}

int sdf_validate_mesh_sharp(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                            const sdf_mesh_sharp* sharp) {
  const int rc = validate_mesh(scene, params, grid, nullptr);
  if (rc != SDF_OK || !sharp) return rc;
  if (sharp->refine < 0 || sharp->refine > 8 || sharp->iterations < 0 || sharp->iterations > 64 ||
      sharp->flags != 0 || sharp->reserved != 0)
    return SDF_E_INVALID_ARG;
  // the placement needs the scene's analytic gradient (sdf_validate_grad)
  const bool plain = sharp->refine == 0 && sharp->iterations == 0;
  return plain || scene->kind == SDF_SCENE_PRIMITIVES ? SDF_OK : SDF_E_UNSUPPORTED;
}

int sdf_mesh_emit_sharp(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                        const sdf_mesh_sharp* sharp, void* workspace, int64_t workspace_bytes,
                        const sdf_mesh_out* out, void* stream) {
  int64_t nbricks = 0;
  int rc = validate_mesh(scene, params, grid, &nbricks);
  if (rc != SDF_OK) return rc;
  if (!out || !mesh_workspace_fits(workspace, workspace_bytes, nbricks)) return SDF_E_INVALID_ARG;
  if (out->max_verts < 0 || out->max_tris < 0) return SDF_E_INVALID_ARG;
  if ((out->max_verts > 0 && !out->verts) || (out->max_tris > 0 && !out->tris))
    return SDF_E_INVALID_ARG;
  rc = sdf_validate_mesh_sharp(scene, params, grid, sharp);
  if (rc != SDF_OK) return rc;
  if (out->max_verts == 0 && out->max_tris == 0) return SDF_OK;   // nothing may be written
  // NULL and (0, 0) are sdf_mesh_emit itself: its kernel
  const bool plain = !sharp || (sharp->refine == 0 && sharp->iterations == 0);
  return mesh_launch(plain ? sdf::kMeshEmit : sdf::kMeshEmitSharp, scene, params, grid, nbricks,
                     workspace, nullptr, out, sharp, stream);
}

int sdf_mesh_emit(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                  void* workspace, int64_t workspace_bytes, const sdf_mesh_out* out,
                  void* stream) {
  return sdf_mesh_emit_sharp(scene, params, grid, nullptr, workspace, workspace_bytes, out, stream);
}

// ---- measures (sdf_abi.h "Measures") ---------------------------------------------
namespace {
// scene, params, grid and flags of a measure call: a mesh's checks, then its own
int validate_measure(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                     int32_t flags, int64_t* nbricks) {
  const int rc = validate_mesh(scene, params, grid, nbricks);
  if (rc != SDF_OK) return rc;
  for (int c = 0; c < 3; ++c)
    if (grid->n[c] > 65536) return SDF_E_INVALID_ARG;
  return (flags & ~SDF_MEASURE_OWNERS) ? SDF_E_INVALID_ARG : SDF_OK;
}
int64_t measure_workspace(int64_t nbricks, int32_t flags) {
  const int rows = sdf::measure_rows((flags & SDF_MEASURE_OWNERS) != 0);
  return sdf::measure_blocks(nbricks) * int64_t(sdf::measure_record(rows)) * int64_t(sizeof(int64_t));
}
}  // namespace

int sdf_validate_measure(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                         int32_t flags) {
  return validate_measure(scene, params, grid, flags, nullptr);
}

int64_t sdf_measure_workspace_bytes(const sdf_grid* grid, int32_t flags) {
  int64_t nbricks = 0;
  const int rc = validate_grid(grid, &nbricks);
  if (rc != SDF_OK) return rc;
  for (int c = 0; c < 3; ++c)
    if (grid->n[c] > 65536) return SDF_E_INVALID_ARG;
  if (flags & ~SDF_MEASURE_OWNERS) return SDF_E_INVALID_ARG;
  return measure_workspace(nbricks, flags);
}

// One validated measure: the scene's plan with the grid, the measure kernel of
// the flags over the bricks, then the combination of its workgroups' records.
int sdf_measure(const sdf_scene* scene, const sdf_params* params, const sdf_grid* grid,
                int32_t flags, void* workspace, int64_t workspace_bytes, int64_t* moments,
                int64_t* counts, void* stream) {
  int64_t nbricks = 0;
  const int rc = validate_measure(scene, params, grid, flags, &nbricks);
  if (rc != SDF_OK) return rc;
  if (!moments || !counts) return SDF_E_INVALID_ARG;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0 ||
      workspace_bytes < measure_workspace(nbricks, flags))
    return SDF_E_INVALID_ARG;
  std::unique_ptr<sdf::RenderPlan> plan(new sdf::RenderPlan());
  const int prc = scene_plan(scene, nullptr, query_params(*params, false), plan.get());
  if (prc != SDF_OK) return prc;
  std::unique_ptr<sdf::MeasureArgs> m(new sdf::MeasureArgs());
  m->a = plan->a;
  for (int i = 0; i < 3; ++i) {
    m->origin[i] = grid->origin[i];
    m->cell[i] = grid->cell[i];
    m->n[i] = grid->n[i];
    m->nb[i] = (grid->n[i] + 7) / 8;
  }
  m->iso = grid->iso;
  m->skip = mesh_skip_bound(*scene, *grid);
  m->nbricks = nbricks;
  m->ws = static_cast<long long*>(workspace);
  m->owners = flags & SDF_MEASURE_OWNERS;
  m->reserved = 0;
  const int lrc = sdf::launch_planned(*plan, sdf::launch_measure_jit, &sdf::RenderUnit::measure, *m,
                                      stream);
  if (lrc != SDF_OK) return lrc;
  const int err = sdf::launch_measure_reduce(m->ws, (int)sdf::measure_blocks(nbricks),
                                             sdf::measure_rows(m->owners != 0), nbricks,
                                             (long long*)moments, (long long*)counts, stream);
  return err == hipSuccess ? SDF_OK : SDF_E_HIP;
}

// ---- gradients (sdf_abi.h "Gradients") -----------------------------------------
static_assert(sizeof(sdf_grad_out) == 24, "sdf_grad_out layout");
namespace {
// scene and params of a gradient call: a query's checks, then the Mandelbulb
int validate_grad(const sdf_scene* scene, const sdf_params* params) {
  if (!scene || !params) return SDF_E_INVALID_ARG;
  const int rc = validate_query(scene, nullptr, query_params(*params, false));
  if (rc != SDF_OK) return rc;
  return scene->kind == SDF_SCENE_PRIMITIVES ? SDF_OK : SDF_E_UNSUPPORTED;
}
int64_t grad_workspace(int64_t n) {
  return sdf::grad_blocks(n) * int64_t(sdf::kGradSlots) * int64_t(sizeof(float));
}
}  // namespace

int sdf_validate_grad(const sdf_scene* scene, const sdf_params* params) {
  return validate_grad(scene, params);
}

int64_t sdf_grad_workspace_bytes(int64_t n) {
  if (n < 0 || n > kMaxQuery) return SDF_E_INVALID_ARG;
  return grad_workspace(n);
}

int sdf_sample_grad(const sdf_scene* scene, const sdf_params* params, const float* points,
                    int64_t n, const float* upstream, const sdf_grad_out* out, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  if (!scene || !params || !out) return SDF_E_INVALID_ARG;
  if (!out->dist && !out->grad_points && !out->grad_prims) return SDF_E_INVALID_ARG;
  if (n < 0 || n > kMaxQuery || (n > 0 && !points)) return SDF_E_INVALID_ARG;
  // n = 0 needs no workspace (sdf_grad_workspace_bytes(0) = 0)
  if (out->grad_prims && n > 0 &&
      (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0 ||
       workspace_bytes < grad_workspace(n)))
    return SDF_E_INVALID_ARG;
  const int rc = validate_grad(scene, params);
  if (rc != SDF_OK) return rc;
  if (n == 0) return SDF_OK;   // nothing to launch, no device needed
  // always the generic, unculled evaluator (the dispatch was validated and is
  // otherwise ignored): no run-time specialised kernel is ever tried
  sdf_params q = query_params(*params, false);
  q.dispatch = SDF_DISPATCH_UNCULLED;
  std::unique_ptr<sdf::RenderPlan> plan(new sdf::RenderPlan());
  const int prc = scene_plan(scene, nullptr, q, plan.get());
  if (prc != SDF_OK) return prc;
  std::unique_ptr<sdf::GradArgs> g(new sdf::GradArgs());
  g->a = plan->a;
  g->points = points;
  g->upstream = upstream;
  g->dist = out->dist;
  g->grad_points = out->grad_points;
  g->rows = out->grad_prims ? static_cast<float*>(workspace) : nullptr;
  g->n = n;
  return sdf::launch_built_in(*plan, &sdf::RenderUnit::grad, *g, stream, out->grad_prims);
}

// ---- caller-supplied rays (sdf_abi.h "Rays") ----------------------------------
namespace {
const sdf_reflect kNoBounce = {0, 1.0f, -1, 0};   // reflect NULL: bounces 0, the composite

// The params a call over a list of rays or points is validated and run with:
// the caller's, with the frame size (a list has none) at sdf_defaults' values;
// `points` have no samples and no output format either.
sdf_params list_params(const sdf_params& p, bool points) {
  sdf_params d;
  sdf_defaults(nullptr, nullptr, nullptr, nullptr, &d, 0, 0);
  sdf_params q = p;
  q.width = d.width;
  q.height = d.height;
  if (points) q.samples = d.samples, q.output_format = d.output_format;
  return q;
}

// A rays call's own checks, and its request validated once: on return under
// the params it runs with, *q, and with no bounce where none was asked.
int validate_rays(sdf::Request& r, const sdf_rays* rays, sdf_params* q) {
  if (!rays || !r.scene || !r.params) return SDF_E_INVALID_ARG;
  if (rays->flags & ~SDF_RAYS_UNIT) return SDF_E_INVALID_ARG;
  if (rays->n < 0 || rays->n > kMaxQuery) return SDF_E_INVALID_ARG;
  if (rays->n > 0 && (!rays->origins || !rays->dirs)) return SDF_E_INVALID_ARG;
  *q = list_params(*r.params, false);
  r.params = q;
  if (!r.reflect) r.reflect = &kNoBounce;
  const int rc = sdf::validate_request(r, sdf::kEnv, false);
  if (rc != SDF_OK) return rc;
  // the caller supplies more rays and averages; a stream has no list of rays
  if (q->samples > 1 || sdf::is_stream(q->output_format)) return SDF_E_UNSUPPORTED;
  return SDF_OK;
}
}  // namespace

int sdf_validate_rays(const sdf_scene* scene, const sdf_light* lights, int32_t nlights,
                      int32_t light_flags, const sdf_material* materials, int32_t nmaterials,
                      const sdf_reflect* reflect, const sdf_environment* env,
                      const sdf_params* params, const sdf_rays* rays) {
  sdf_params q;
  sdf::Request r = {scene,   nullptr, lights, nlights, light_flags, materials, nmaterials,
                    reflect, env,     params, nullptr};
  return validate_rays(r, rays, &q);
}

int sdf_render_rays(const sdf_scene* scene, const sdf_light* lights, int32_t nlights,
                    int32_t light_flags, const sdf_material* materials, int32_t nmaterials,
                    const sdf_reflect* reflect, const sdf_environment* env,
                    const sdf_params* params, const sdf_rays* rays, void* rgba, int32_t* steps,
                    void* stream) {
  sdf_params q;
  sdf::Request r = {scene,   nullptr, lights, nlights, light_flags, materials, nmaterials,
                    reflect, env,     params, nullptr};
  int rc = validate_rays(r, rays, &q);
  if (rc != SDF_OK) return rc;
  if (rays->n == 0) return SDF_OK;   // nothing to launch, no device needed
  if (!rgba) return SDF_E_INVALID_ARG;
  // the scene's plan under light 0 and material 0, with the uniforms of a
  // reflect launch (an env launch where one is asked) and the ray buffers in
  // place of a frame's geometry
  std::unique_ptr<sdf::RenderPlan> plan(new sdf::RenderPlan());
  rc = scene_plan(scene, nullptr, q, plan.get(), &lights[0], &materials[0]);
  if (rc != SDF_OK) return rc;
  fill_plan(*plan, r, std::max(sdf::route(r), sdf::kReflect));
  std::unique_ptr<sdf::RaysArgs> a(new sdf::RaysArgs());
  a->a = plan->a;
  a->a.rgba = rgba;
  a->a.steps = steps;
  a->l = plan->lights;
  a->m = plan->materials;
  a->r = plan->reflect;
  a->e = plan->env;
  a->in0 = rays->origins;
  a->in1 = rays->dirs;
  a->n = rays->n;
  a->flags = rays->flags;
  return sdf::launch_planned(*plan, sdf::launch_rays_jit, &sdf::RenderUnit::rays, *a, stream);
}

int sdf_camera_rays(const sdf_camera* camera, const sdf_params* params, float* origins,
                    float* dirs, void* stream) {
  if (!camera || !params || (!origins && !dirs)) return SDF_E_INVALID_ARG;
  const sdf_params q = query_params(*params, true);
  const int rc = validate_query(nullptr, camera, q);
  if (rc != SDF_OK) return rc;
  if (params->samples > 1) return SDF_E_UNSUPPORTED;   // one ray per pixel
  if (no_device()) return SDF_E_NO_DEVICE;
  // the hoisted camera and the quad mapping of a render of this frame size;
  // no scene: the precision alone picks the kernel (variant 0, never JIT)
  std::unique_ptr<sdf::RenderPlan> plan(new sdf::RenderPlan());
  std::unique_ptr<sdf::RaysArgs> a(new sdf::RaysArgs());
  plan->exact = q.precision == SDF_PRECISION_EXACT;
  sdf::plan_view(plan.get(), *camera, q.width, q.height);
  a->a = plan->a;
  a->out0 = origins;
  a->out1 = dirs;
  return sdf::launch_built_in(*plan, &sdf::RenderUnit::camera_rays, *a, stream);
}

// ---- shading at caller-supplied points (sdf_abi.h "Points") --------------------
static_assert(sizeof(sdf_points) == 48, "sdf_points layout");
static_assert(sizeof(sdf_point_shade) == 40, "sdf_point_shade layout");

namespace {
// A points call's own checks, and its request validated once: on return under
// the params it runs with, *q.
int validate_points(sdf::Request& r, const sdf_points* pts, sdf_params* q) {
  if (!pts || !r.scene || !r.params) return SDF_E_INVALID_ARG;
  if ((pts->flags & ~SDF_POINTS_EYE) || pts->reserved != 0) return SDF_E_INVALID_ARG;
  if (pts->n < 0 || pts->n > kMaxQuery || (pts->n > 0 && !pts->points)) return SDF_E_INVALID_ARG;
  if (!(pts->lift >= 0.0f && pts->lift <= 1e15f)) return SDF_E_INVALID_ARG;
  if (pts->flags & SDF_POINTS_EYE)
    for (int c = 0; c < 3; ++c)
      if (!(std::fabs(pts->eye[c]) <= 1e15f)) return SDF_E_INVALID_ARG;
  *q = list_params(*r.params, true);
  r.params = q;
  return sdf::validate_request(r, sdf::kMaterials, false);
}
}  // namespace

int sdf_validate_points(const sdf_scene* scene, const sdf_light* lights, int32_t nlights,
                        int32_t light_flags, const sdf_material* materials, int32_t nmaterials,
                        const sdf_params* params, const sdf_points* pts) {
  sdf_params q;
  sdf::Request r = {scene,   nullptr, lights, nlights, light_flags, materials, nmaterials,
                    nullptr, nullptr, params, nullptr};
  return validate_points(r, pts, &q);
}

int sdf_shade_points(const sdf_scene* scene, const sdf_light* lights, int32_t nlights,
                     int32_t light_flags, const sdf_material* materials, int32_t nmaterials,
                     const sdf_params* params, const sdf_points* pts,
                     const sdf_point_shade* out, void* stream) {
  if (!out) return SDF_E_INVALID_ARG;
  if (!out->rgba && !out->ao && !out->shadow && !out->material && !out->steps)
    return SDF_E_INVALID_ARG;
  // the kernels store a point's colour as one 16-byte word
  if (reinterpret_cast<uintptr_t>(out->rgba) % 16 != 0) return SDF_E_INVALID_ARG;
  sdf_params q;
  sdf::Request r = {scene,   nullptr, lights, nlights, light_flags, materials, nmaterials,
                    nullptr, nullptr, params, nullptr};
  int rc = validate_points(r, pts, &q);
  if (rc != SDF_OK) return rc;
  if (pts->n == 0) return SDF_OK;   // nothing to launch, no device needed
  // the scene's plan (scene blocks, culling bounds, march and shading parameters,
  // dispatch; no camera, no frame, no outputs) under light 0 and material 0,
  // with the lights and the table of a materials launch and the point buffers
  std::unique_ptr<sdf::RenderPlan> plan(new sdf::RenderPlan());
  rc = scene_plan(scene, nullptr, q, plan.get(), &lights[0], &materials[0]);
  if (rc != SDF_OK) return rc;
  fill_plan(*plan, r, sdf::kMaterials);
  std::unique_ptr<sdf::PointsArgs> a(new sdf::PointsArgs());
  a->a = plan->a;
  // the occlusion taps run only for an output that needs them
  if (!out->rgba && !out->ao) a->a.ao_taps = 0;
  a->l = plan->lights;
  a->m = plan->materials;
  a->points = pts->points;
  a->normals = pts->normals;
  a->rgba = out->rgba;
  a->ao = out->ao;
  a->shadow = out->shadow;
  a->material = out->material;
  a->steps = out->steps;
  a->n = pts->n;
  for (int i = 0; i < 3; ++i) a->eye[i] = (pts->flags & SDF_POINTS_EYE) ? pts->eye[i] : 0.0f;
  a->lift = pts->lift;
  a->flags = pts->flags;
  a->reserved = 0;
  return sdf::launch_planned(*plan, sdf::launch_points_jit, &sdf::RenderUnit::points, *a, stream);
}

int sdf_jit_count(void) { return sdf::jit_compiled_count(); }

// SDF_KERNEL_ID_EXACT / _FAST: written by sdf3d_amd/build.py (kernel_id())
#include "kernel_id.inc"

const char* sdf_kernel_id(int32_t precision) {
  if (precision == SDF_PRECISION_EXACT) return SDF_KERNEL_ID_EXACT;
  if (precision == SDF_PRECISION_FAST) return SDF_KERNEL_ID_FAST;
  return nullptr;
}

int sdf_scene_bounds(const sdf_scene* scene, float* bounds, float* cluster,
                     int32_t* cluster_first) {
  if (!scene || !bounds || !cluster || !cluster_first) return SDF_E_INVALID_ARG;
  const int rc = validate_scene(*scene);
  if (rc != SDF_OK) return rc;
  if (scene->kind != SDF_SCENE_PRIMITIVES) return SDF_E_UNSUPPORTED;
  std::unique_ptr<sdf::KernelArgs> a(new sdf::KernelArgs());
  prepare_bounds(*scene, *a);
  std::memcpy(bounds, a->bound, sizeof(a->bound));
  std::memcpy(cluster, a->cluster, sizeof(a->cluster));
  *cluster_first = a->cluster_first;
  return SDF_OK;
}

namespace {
int decode_parts(const void* parts, int32_t nparts, int64_t part_stride, const sdf_tiling* tilings,
                 const int64_t* used, int32_t width, int32_t height, void* frame, uint32_t* status,
                 void* stream) {
  if (!parts || !frame || !tilings || nparts <= 0 || nparts > SDF_MAX_DECODE_PARTS ||
      width <= 0 || height <= 0)
    return SDF_E_INVALID_ARG;
  sdf::DecodeParts d{};
  d.status = status;
  if (used)
    for (int r = 0; r < nparts; ++r) d.used[r] = used[r] < 0 ? -1 : used[r];
  d.nparts = nparts;
  d.width = width;
  d.height = height;
  d.part_stride = part_stride;
  for (int r = 0; r < nparts; ++r) {
    const sdf_tiling& t = tilings[r];
    const int rows = count_rows(height, t);
    if (rows < 0 || t.flags != 0) return SDF_E_INVALID_ARG;
    // every part's stream must fit its pitch
    const int64_t n = int64_t((width + 7) / 8) * ((rows + 7) / 8);
    if ((int64_t)sdf::TilesLayout(n).stream_end > part_stride) return SDF_E_INVALID_ARG;
    d.rows[r] = rows;
    d.first_block[r] = t.first_block;
    d.block_stride[r] = t.block_stride;
    d.block_rows[r] = t.block_rows;
    d.chunk_rows[r] = t.block_rows * sdf::tiling_run(t);
    d.run_gap_rows[r] = sdf::tiling_gap_rows(t);
  }
  const int err = sdf::launch_tiles_decode(d, frame, parts, stream);
  return err == hipSuccess ? SDF_OK : SDF_E_HIP;
}
}  // namespace

int sdf_tiles_decode_tilings(const void* parts, int32_t nparts, int64_t part_stride,
                             const sdf_tiling* tilings, int32_t width, int32_t height,
                             void* frame, void* stream) {
  return decode_parts(parts, nparts, part_stride, tilings, nullptr, width, height, frame, nullptr,
                      stream);
}

int sdf_tiles_decode_checked(const void* parts, int32_t nparts, int64_t part_stride,
                             const sdf_tiling* tilings, const int64_t* used, int32_t width,
                             int32_t height, void* frame, uint32_t* status, void* stream) {
  if (status)
    return decode_parts(parts, nparts, part_stride, tilings, used, width, height, frame, status,
                        stream);
  // synchronous: status words of the library's own (pinned host memory the
  // device writes), read once the decode is done
  if (nparts <= 0 || nparts > SDF_MAX_DECODE_PARTS) return SDF_E_INVALID_ARG;
  uint32_t* st = nullptr;
  if (hipHostMalloc((void**)&st, sizeof(uint32_t) * nparts, hipHostMallocDefault) != hipSuccess)
    return SDF_E_HIP;
  std::memset(st, 0, sizeof(uint32_t) * nparts);
  int rc = decode_parts(parts, nparts, part_stride, tilings, used, width, height, frame, st, stream);
  if (rc == SDF_OK && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = SDF_E_HIP;
  if (rc == SDF_OK)
    for (int r = 0; r < nparts; ++r)
      if (st[r]) rc = SDF_E_COMM;
  (void)hipHostFree(st);
  return rc;
}

int sdf_tiles_decode(const void* parts, int32_t nparts, int64_t part_stride, int32_t width,
                     int32_t height, int32_t block_rows, void* frame, void* stream) {
  if (nparts <= 0 || nparts > SDF_MAX_DECODE_PARTS || block_rows <= 0) return SDF_E_INVALID_ARG;
  sdf_tiling t[SDF_MAX_DECODE_PARTS];
  for (int r = 0; r < nparts; ++r) t[r] = {block_rows, r, nparts, 0, 1};
  return sdf_tiles_decode_tilings(parts, nparts, part_stride, t, width, height, frame, stream);
}

int sdf_deinterleave(const void* parts, int32_t nparts, int32_t part_stride_rows,
                     int32_t width, int32_t height, int32_t block_rows, int32_t format,
                     void* frame, void* stream) {
  const int bpp = sdf_format_bytes(format);
  if (bpp < 0 || !parts || !frame || nparts <= 0 || width <= 0 || height <= 0 ||
      block_rows <= 0)
    return SDF_E_INVALID_ARG;
  // every part must hold its owned rows
  for (int r = 0; r < nparts; ++r) {
    const sdf_tiling t = {block_rows, r, nparts, 0, 1};
    if (count_rows(height, t) > part_stride_rows) return SDF_E_INVALID_ARG;
  }
  const int err =
      format == SDF_FORMAT_RGB32F
          ? sdf::launch_deinterleave_rgb(parts, nparts, part_stride_rows, width, height,
                                         block_rows, frame, stream)
          : sdf::launch_deinterleave(parts, nparts, part_stride_rows, width * bpp, height,
                                     block_rows, frame, stream);
  return err == hipSuccess ? SDF_OK : SDF_E_HIP;
}

int sdf_heatmap(const int32_t* steps, int32_t count, int32_t which, int32_t max_steps,
                int32_t format, void* out, void* stream) {
  if (count < 0 || which < 0 || which > 2 || max_steps < 0 || sdf_format_bytes(format) < 0 ||
      format == SDF_FORMAT_SHADE32F)   // colours only
    return SDF_E_INVALID_ARG;
  if (count == 0) return SDF_OK;
  if (!steps || !out) return SDF_E_INVALID_ARG;
  const int err = sdf::launch_heatmap(steps, count, which, max_steps, format, out, stream);
  return err == hipSuccess ? SDF_OK : SDF_E_HIP;
}

const char* sdf_strerror(int code) {
  switch (code) {
    case SDF_OK: return "success";
    case SDF_E_INVALID_ARG: return "invalid argument";
    case SDF_E_UNSUPPORTED: return "unsupported request";
    case SDF_E_HIP: return "HIP runtime error";
    case SDF_E_NO_DEVICE: return "no HIP device available";
    case SDF_E_COMM: return "RCCL unavailable or a collective failed";
    case SDF_E_TIMEOUT: return "frame driver wait timed out";
    default: return "unknown error";
  }
}

}  // extern "C"
