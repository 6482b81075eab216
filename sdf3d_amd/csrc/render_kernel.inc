// render_kernel.inc -- the per-pixel SDF sphere-tracing kernel for gfx950.
//
// Included by render_exact.hip (SDF_EXACT = 1, compiled -ffp-contract=off with
// IEEE div/sqrt: the same fp32 operation sequence as the fragment shader, so
// the output is bit-comparable with the CPU oracle) and by render_fast.hip
// (SDF_EXACT = 0: FMA contraction, v_sqrt/v_rcp/v_rsq, min/max instructions).
//
// What one lane computes = fragment-stage main() of the reference,
// /root/reference/Code/shader/voxel_fragment.frag:160-211, for one pixel:
//   ray generation (:191-192, pixel -> quad from voxel_geometry.geom:26-52)
//   raymarch (:86-103) -> normal (:134-155, or tetrahedral) -> Blinn-Phong
//   (:200-204) -> soft shadow (:105-132, :205) -> [AO] -> colour (:206-210).
//
// Mapping: one lane = one pixel; one wave64 = an 8x8 pixel tile (rays of a
// tile are coherent, so the march loop's exec mask stays full longer and the
// wave leaves the loop as soon as its last lane converges); a workgroup is
// kWgWaves tiles side by side (kernel_args.h: one).  Scene constants come from
// the kernel-argument segment with scalar loads.  The only HBM traffic is the
// 16-byte float4 store per pixel (row-contiguous 128-byte segments per tile row).
//
// Device code only: the four render units include their host launchers
// behind this file (render_launch.inc); hipRTC compiles this file alone.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#else
// compiled at run time by hipRTC for one scene signature (jit.cpp)
#define INFINITY __builtin_inff()
#endif

#include "kernel_args.h"
#include "wave_bits.h"
#include "shade.h"
#if SDF_EXACT
// cr_math.h's one-compare square-root guard (cr_sqrt exact for every finite
// argument) in the CSG units: there sdf_validate's working range (every
// coordinate, size and distance <= 1e15) keeps every squared length below
// ~1e33, so +INF never reaches it.  The Mandelbulb unit's orbit may overflow:
// the full range test (every x).
#if !defined(SDF_CRM_SQRT_GUARD) && !defined(SDF_TU_BULB)
#define SDF_CRM_SQRT_GUARD 1
#endif
#include "cr_math.h"
#endif

#ifndef SDF_EXACT
#error "SDF_EXACT must be 0 or 1"
#endif

// Waves per SIMD the render kernels are built for (the VGPR budget): 8 =
// 64 VGPRs.  Overridable per build for occupancy experiments.
#ifndef SDF_WAVES_PER_EU
#define SDF_WAVES_PER_EU 8
#endif

// Stage ablation (tools/ablate.py): 1 skips the normal's taps, so a frame's
// time splits into primary march, normal, AO and shadow.  Experiment builds
// only (tools/flag_variant.py defines SDF_EXPERIMENT).
#ifndef SDF_ABLATE_NO_NORMAL
#define SDF_ABLATE_NO_NORMAL 0
#endif
#if SDF_ABLATE_NO_NORMAL && !defined(SDF_EXPERIMENT)
#error "SDF_ABLATE_NO_NORMAL renders wrong pixels: experiment builds only"
#endif

// SDF_TU_BULB 1: this translation unit holds the Mandelbulb scene's kernels
// alone (render_{fast,exact}_bulb.hip), built with a scheduler of its own
// (build.py); 0: every other scene.
#ifndef SDF_TU_BULB
#define SDF_TU_BULB 0
#endif
#if SDF_EXACT
#define SDF_NS exact_impl
#else
#define SDF_NS fast_impl
#endif

namespace sdf {
namespace SDF_NS {

// The kernel's by-value KernelArgs lives in the kernarg segment; reading it
// through an address_space(4) pointer keeps every uniform access a scalar
// (s_load) read instead of a per-lane scratch copy of the 2.1 KB struct.
#define KARG __attribute__((address_space(4)))
typedef const KARG KernelArgs KA;
typedef const KARG float* KF;

// Culling bounds in VGPRs (fast precision: its SGPRs hold the primitive
// parameters) or as uniform kernel-argument values (exact precision: its
// longer sequences need the VGPRs -- with the bounds in them the CSG8 kernel
// spilled 68 bytes per lane at 8 waves, 170 MB of scratch writes per 4K
// launch; without, none, and C3/C4 exact run 1-21 % faster).
constexpr bool kBoundsInVgprs = !SDF_EXACT;

struct V3 {
  float x, y, z;
};

// Move a uniform value into a VGPR.  Used for values the march loops read
// rarely (culling bounds), so the SGPR file keeps the hot primitive
// parameters without spilling or re-loading them inside the loops.
__device__ __forceinline__ float to_vgpr(float x) {
  float y;
  asm volatile("v_mov_b32 %0, %1" : "=v"(y) : "s"(x));
  return y;
}

// A zero the compiler must treat as per-lane.  Indexing kernel arguments with
// it turns their loads into vector loads (global_load_dwordx4, every lane the
// same address) issued together, whose results land in VGPRs -- instead of a
// chain of scalar load / wait / v_mov per value at wave start.
__device__ __forceinline__ int lane_zero() {
  int z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
}

template <int... I>
struct Seq {};
template <int N, int... I>
struct MakeSeqImpl : MakeSeqImpl<N - 1, N - 1, I...> {};
template <int... I>
struct MakeSeqImpl<0, I...> {
  using type = Seq<I...>;
};
template <int N>
using MakeSeq = typename MakeSeqImpl<N>::type;

__device__ __forceinline__ V3 mk(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 muls(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

#if SDF_EXACT
// GLSL 4.60 select semantics (SURVEY.md Appendix A); IEEE sqrt and division.
__device__ __forceinline__ float gmin(float x, float y) { return y < x ? y : x; }
__device__ __forceinline__ float gmax(float x, float y) { return x < y ? y : x; }
// sqrt: IEEE (cr_math.h cr_sqrt: a v_rsq-based fast path proven on all 2^32
// inputs, tests/test_gpu_crmath.py); division: the compiler's IEEE sequence.
__device__ __forceinline__ float fsqrt(float x) { return crm::cr_sqrt(x); }
__device__ __forceinline__ float fdiv(float a, float b) { return a / b; }
// 1 / sqrt(x), both roundings IEEE as the oracle's 1 / SQRT(x): rcp_fast is
// the IEEE reciprocal on [2^-100, 2^100) (checked on all of it), which holds
// sqrt(x) for the only caller, the Mandelbulb's x = k3 in [1e-30, 4]
__device__ __forceinline__ float frsqrt(float x) { return crm::rcp_fast(crm::cr_sqrt(x)); }
// log correctly rounded to fp32, as the oracle's cr_logf (oracle/sdf_oracle.c),
// so exact precision does not inherit ocml's last-ulp choices: cr_math.h
// cr_log (checked on all 2^32 inputs).  pow: shade.h spec_pow (fp64, rounded
// once, as the oracle's cr_powf).
__device__ __forceinline__ float flog(float x) { return crm::cr_log(x); }
// Exact precision's divisions by Markstein's steps instead of the IEEE
// sequence (v_div_scale x2, v_rcp, 5 fma, v_div_fmas / v_div_fixup through
// VCC): correctly rounded, proven in cr_math.h, guarded to their domain.
//   normalize's three divisions, one shared reciprocal (div3): C4 exact
//     2.8-2.9 % faster than without, C5 1.3 %
//   the Mandelbulb's (p - c) / scale from the host's RN(1/scale), three
//     divisions per DE evaluation (BulbScene::local): C5 exact 10-11 % faster
//   the pixel's quad coordinates (2x+1)/W, (2y+1)/H (div_refined with the
//     host's RN(1/W), no guard: integers in range)
//   the capsule's h (sd_capsule) and the smooth-min's h (smin)
// (all bit-exact at 4K, profiles/r05_ab_exact_C4.json, r05_ab_divisions_C5.json).
// The DE's final division by dz and the shadow march's h^2 / (2 h_prev) stay
// IEEE: div_one measured no faster there (DESIGN.md Appendix A).
__device__ __forceinline__ V3 normalize(V3 a) {
  float l = fsqrt(dot(a, a));
  crm::div3(a.x, a.y, a.z, l);
  return a;
}
#else
// Hardware min/max (differ from the GLSL select only for a NaN first
// operand), 1-ulp v_sqrt, v_rcp-based division, v_rsq normalisation.
__device__ __forceinline__ float gmin(float x, float y) { return fminf(x, y); }
__device__ __forceinline__ float gmax(float x, float y) { return fmaxf(x, y); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fdiv(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float frsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float flog(float x) {
  return __builtin_amdgcn_logf(x) * 0.693147180559945f;
}
__device__ __forceinline__ V3 normalize(V3 a) {
  float r = frsqrt(dot(a, a));
  return mk(a.x * r, a.y * r, a.z * r);
}
#endif

__device__ __forceinline__ float gclamp(float x, float a, float b) { return gmin(gmax(x, a), b); }

// min / max inside the primitive SDFs (box, round box, cylinder, the
// capsule's clamp).  Exact precision: the hardware v_max_f32 / v_min_f32 /
// v_max3_f32 equal the GLSL select there: no operand is
// NaN (sdf_validate's working range keeps every coordinate, square and
// distance finite) and none is -0 -- |v| - b and sqrt(.) - r are never -0
// (x - y = -0 needs x = -0), and a max of such values is one of them -- so
// the only pairs where select and hardware differ, a NaN or (+0, -0), never
// occur.  The capsule's h = dot(pa, ba) / dot(ba, ba) may be -0; the select
// keeps -0 where the hardware gives +0, and h only enters pa - ba h, whose
// components are then +-0 alike and square to +0: the same length.
#if SDF_EXACT
__device__ __forceinline__ float hw_max(float x, float y) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ float hw_min(float x, float y) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ float hw_max3(float x, float y, float z) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}
__device__ __forceinline__ float pmax(float x, float y) { return hw_max(x, y); }
__device__ __forceinline__ float pmin(float x, float y) { return hw_min(x, y); }
__device__ __forceinline__ float pmax3(float x, float y, float z) { return hw_max3(x, y, z); }
#else
__device__ __forceinline__ float pmax(float x, float y) { return gmax(x, y); }
__device__ __forceinline__ float pmin(float x, float y) { return gmin(x, y); }
__device__ __forceinline__ float pmax3(float x, float y, float z) { return gmax(x, gmax(y, z)); }
#endif
__device__ __forceinline__ float length(V3 a) { return fsqrt(dot(a, a)); }

// ---- primitives (formulas frozen in DESIGN.md "Scene spec") ---------------
// `q` is the host-prepared parameter block of one primitive (sdf_abi.cpp
// prepare_prims): raw parameters plus uniform-only derived values computed
// once per frame in fp32 with the same operations the oracle performs per
// call (b - r, b - a, dot(ba, ba)), so exact precision stays bit-identical.
// Q is a kernarg pointer (generic kernel) or a register array (fixed scenes).

// x / d with the host's 1 / d beside it (grad_kernel.inc's capsule)
#if SDF_EXACT
#define DIVK(x, d, inv) ((x) / (d))
#else
#define DIVK(x, d, inv) ((x) * (inv))
#endif

// sphereSDF, voxel_fragment.frag:54-64: c.xyz, r
template <class Q>
__device__ __forceinline__ float sd_sphere(V3 p, const Q& q) {
  return length(sub(p, mk(q[0], q[1], q[2]))) - q[3];
}
// planeSDF, voxel_fragment.frag:66-71 (n = (0,1,0), h = 0 gives p.y): n.xyz, h
template <class Q>
__device__ __forceinline__ float sd_plane(V3 p, const Q& q) {
  return dot(p, mk(q[0], q[1], q[2])) + q[3];
}
#if !SDF_EXACT
// 2 max(q, 0) = q + |q| exactly (q + q is a doubling, q + -q is +0), and
// sqrt(4 S) = 2 sqrt(S) exactly, so length(max(q, 0)) = 0.5 sqrt(sum (q+|q|)^2)
// bit for bit -- with full-rate adds instead of half-rate v_max_f32.
__device__ __forceinline__ float pos2(float q) { return q + fabsf(q); }
#endif
__device__ __forceinline__ float box_core(V3 v, float bx, float by, float bz) {
  float qx = fabsf(v.x) - bx, qy = fabsf(v.y) - by, qz = fabsf(v.z) - bz;
  float inside = pmin(pmax3(qx, qy, qz), 0.0f);
#if SDF_EXACT
  float outside = length(mk(pmax(qx, 0.0f), pmax(qy, 0.0f), pmax(qz, 0.0f)));
  return outside + inside;
#else
  return fmaf(0.5f, length(mk(pos2(qx), pos2(qy), pos2(qz))), inside);
#endif
}
// c.xyz, b.xyz
template <class Q>
__device__ __forceinline__ float sd_box(V3 p, const Q& q) {
  return box_core(sub(p, mk(q[0], q[1], q[2])), q[3], q[4], q[5]);
}
// c.xyz, (b - r).xyz, r
template <class Q>
__device__ __forceinline__ float sd_round_box(V3 p, const Q& q) {
  return box_core(sub(p, mk(q[0], q[1], q[2])), q[3], q[4], q[5]) - q[6];
}
// c.xyz, R, r
template <class Q>
__device__ __forceinline__ float sd_torus(V3 p, const Q& q) {
  V3 v = sub(p, mk(q[0], q[1], q[2]));
  float qx = fsqrt(v.x * v.x + v.z * v.z) - q[3];
  return fsqrt(qx * qx + v.y * v.y) - q[4];
}
// a.xyz, (b - a).xyz, r, dot(ba, ba), 1 / dot(ba, ba)
//
// Exact precision: h = clamp(dot(pa, ba) / dot(ba, ba), 0, 1) as the
// quotient of the CLAMPED numerator med3(n, 0, b) by cr_math.h div_refined
// (the host's RN(1/b), one Markstein step: the proof is at div_refined)
// instead of the IEEE division (11 VALU, a v_rcp among them) and the clamp.
// The same bits: for n <= 0 both give +0 (the capsule's pa - ba h squares a
// -0 alike, see pmax); for 0 < n < b the quotient is RN(n/b) either way and
// lies in (0, 1]; for n >= b both give RN(b/b) = 1.  div_refined's domain:
// b = dot(ba, ba) in [2^-30, 2^30) -- sdf_validate's capsule length range
// [2^-15, 2^15) -- and a numerator 0 or >= 2^-60 (lanes with a smaller one
// take the IEEE path).  tools/block_counts.py: 9 capsule evaluations per
// wave on C4.  Fast precision multiplies by the host's 1 / dot(ba, ba).
template <class Q>
__device__ __forceinline__ float sd_capsule(V3 p, const Q& q) {
  V3 pa = sub(p, mk(q[0], q[1], q[2]));
  V3 ba = mk(q[3], q[4], q[5]);
#if SDF_EXACT
  const float n = dot(pa, ba);
  const float a = __builtin_amdgcn_fmed3f(n, 0.0f, q[7]);
  float h = crm::div_refined(a, q[7], q[8]);
  const bool ok = (__float_as_uint(a) << 1) - 1u >= (0x21800000u << 1) - 1u;
  if (crm::any_lane(!ok)) {
    SDF_CRM_COLD();
    if (!ok) h = pmin(pmax(n / q[7], 0.0f), 1.0f);
  }
#else
  float h = pmin(pmax(dot(pa, ba) * q[8], 0.0f), 1.0f);
#endif
  return length(sub(pa, muls(ba, h))) - q[6];
}
// c.xyz, r, half height
template <class Q>
__device__ __forceinline__ float sd_cylinder(V3 p, const Q& q) {
  V3 v = sub(p, mk(q[0], q[1], q[2]));
  float dx = fsqrt(v.x * v.x + v.z * v.z) - q[3];
  float dy = fabsf(v.y) - q[4];
  float inside = pmin(pmax(dx, dy), 0.0f);
#if SDF_EXACT
  float ox = pmax(dx, 0.0f), oy = pmax(dy, 0.0f);
  return inside + fsqrt(ox * ox + oy * oy);
#else
  const float ox = pos2(dx), oy = pos2(dy);   // 2 max(., 0), see box_core
  return fmaf(0.5f, fsqrt(ox * ox + oy * oy), inside);
#endif
}

// Polynomial smooth-min: equals min(a,b) exactly when |a-b| >= k.
// `kk` is k (exact precision) or k/4 (fast precision; sdf_abi.cpp stores it
// in p[11]), `ik` = 1/k.
#if SDF_EXACT
// The hardware v_max_f32 / v_min_f32 where they provably equal the GLSL
// select: operands never NaN (or NaN only where the select keeps the other
// operand too) and never the (+0, -0) pair the select orders differently
// (the hardware's answers on the pairs relied on: tests/test_gpu_crmath.py
// minmax).  They serve the smooth-min's max and min and the shadow march's
// max / min: C4 exact 0.8-1.4 % faster at 3 poses, bit-identical
// (profiles/r04_ab_minmax_exact_C4.json).
// h = max(k - |a-b|, 0) / k by cr_math.h div_scaled (`ik` = RN(1/(k sc)),
// `sc` = 2^s, prepared by the host in p[10], p[9]): 4 instructions instead of
// the IEEE sequence's 11, and the same result bit for bit (h*h is what
// counts; cr_math.h and tests/test_gpu_crmath.py)
// HW: b is a primitive value that is never -0 (every kind but the plane:
// length(.) - r, box, torus, capsule, cylinder), so the hardware minimum
// (-0 below +0, tests/test_gpu_crmath.py) equals the select gmin(a, b)
// h by cr_math.h smin_h -- the subtraction, the max and the scaling
// as one clamped FMA -- and the product h h k 0.25 as h h (k/4) with the
// host's exact k/4: 9 VALU per smooth union instead of 12 (tools/
// block_counts.py), bit-identical.  The second rests on sdf_validate's
// smooth k >= 2^-64: whenever h > 0, h >= 2^-25 (k - |a - b| is either exact
// by Sterbenz, hence >= ulp(k)/2, or above k/2), so h h k / 4 >= 2^-116 is a
// normal number and RN(RN(hh k) 0.25) = RN(hh k) / 4 = RN(hh (k/4)); the
// same bound keeps n' sc >= 2^-47, far inside smin_h's Markstein domain.
// `k4` = k/4, `ik` = RN(1/(k sc)), `sc`, `ksc` = k sc (sdf_abi.cpp prepare_prims).
template <bool HW = false>
__device__ __forceinline__ float smin(float a, float b, float k4, float ik, float sc, float ksc) {
  const float h = crm::smin_h(a - b, sc, ksc, ik);
  if constexpr (HW) return hw_min(a, b) - h * h * k4;
  return gmin(a, b) - h * h * k4;
}
#else
// The scene accumulator's minimum as one v_min_f32.  fminf would be the same
// instruction, but LLVM must first quiet a possible signalling NaN in an
// operand it cannot prove canonical (a loop-carried or cross-block d), which
// costs a v_max_f32 d, d, d per combine.  The hardware minimum already
// returns the non-NaN operand, as fminf does.
__device__ __forceinline__ float acc_min(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// h = max(k - |a-b|, 0)/k = max(1 - |a-b|/k, 0); result min(a,b) - h^2 (k/4)
// (h <= 1 always since ik > 0: the max folds into the FMA's clamp modifier,
// which also maps NaN to 0 as fmaxf(NaN, 0) does)
template <bool HW = false>
__device__ __forceinline__ float smin(float a, float b, float kk, float ik, float, float) {
  float h = fminf(fmaxf(fmaf(-fabsf(a - b), ik, 1.0f), 0.0f), 1.0f);
  return fmaf(-(h * h), kk, acc_min(a, b));
}
#endif
// parameter slots holding smin's `kk` (k/4), `ik`, `sc` and `ksc` in a
// prepared primitive block (sdf_abi.cpp prepare_prims)
#define SMIN_K(pr) ((pr).p[11])
#if SDF_EXACT
#define SMIN_IK(pr) ((pr).p[10])
#define SMIN_SC(pr) ((pr).p[9])
#define SMIN_KSC(pr) ((pr).k)
#else
#define SMIN_IK(pr) ((pr).reserved)
#define SMIN_SC(pr) (1.0f)
#define SMIN_KSC(pr) (1.0f)
#endif

template <class Q>
__device__ __forceinline__ float prim_sdf(int kind, V3 p, const Q& q) {
  switch (kind) {
    case SDF_PRIM_SPHERE: return sd_sphere(p, q);
    case SDF_PRIM_PLANE: return sd_plane(p, q);
    case SDF_PRIM_BOX: return sd_box(p, q);
    case SDF_PRIM_ROUND_BOX: return sd_round_box(p, q);
    case SDF_PRIM_TORUS: return sd_torus(p, q);
    case SDF_PRIM_CAPSULE: return sd_capsule(p, q);
    default: return sd_cylinder(p, q);
  }
}

template <bool HW = false>
__device__ __forceinline__ float combine(int op, float d, float v, float k, float ik, float sc,
                                        float ksc) {
  switch (op) {
#if SDF_EXACT
    case SDF_OP_UNION: return gmin(d, v);          // voxel_fragment.frag:77-78
#else
    case SDF_OP_UNION: return acc_min(d, v);
#endif
    case SDF_OP_SMOOTH_UNION: return smin<HW>(d, v, k, ik, sc, ksc);
    case SDF_OP_SUBTRACT: return gmax(d, -v);
    case SDF_OP_INTERSECT: return gmax(d, v);
    case SDF_OP_SMOOTH_SUBTRACT: return -smin(-d, v, k, ik, sc, ksc);
    default: return -smin(-d, -v, k, ik, sc, ksc);
  }
}

// One primitive of the material fold (sdf_abi.h "Materials"): the running
// material m[9] (amb, dif, ref) moves towards the primitive's `mi` by the
// weight t its operator gives at the running distance d and the primitive's
// value v, before `combine` advances d.  (a, b) are the arguments combine
// hands to min / smin; a hard operator selects (b < a: the primitive owns the
// surface, the earlier owner keeps a tie), a smooth one blends with the
// smooth-min's own h.  Exact precision forms h with an IEEE division from
// k = 4 (k/4) -- exact, sdf_validate keeps k in [2^-64, 1e15] -- because
// crm::smin_h is only proven to give the right h h; fast precision's h is its
// smin's clamped FMA.  d = +-INF (before primitive 0) gives h = 0 and t = 0
// or 1 without a NaN.  Evaluated once per pixel, so none of this is tuned;
// a wave whose lanes all keep their owner skips the nine updates.
__device__ __forceinline__ void material_step(int op, float d, float v, float k4, float ik, KF mi,
                                              float (&m)[9]) {
  const bool smooth =
      op == SDF_OP_SMOOTH_UNION || op == SDF_OP_SMOOTH_SUBTRACT || op == SDF_OP_SMOOTH_INTERSECT;
  const float a = (op == SDF_OP_UNION || op == SDF_OP_SMOOTH_UNION) ? d : -d;
  const float b = (op == SDF_OP_INTERSECT || op == SDF_OP_SMOOTH_INTERSECT) ? -v : v;
  const bool nearer = b < a;
  float t = nearer ? 1.0f : 0.0f;
  if (smooth) {
#if SDF_EXACT
    (void)ik;
    const float k = 4.0f * k4;
    const float h = gmax(k - fabsf(a - b), 0.0f) / k;
#else
    (void)k4;
    const float h = fminf(fmaxf(fmaf(-fabsf(a - b), ik, 1.0f), 0.0f), 1.0f);
#endif
    t = material_weight(h, nearer);
  }
  if (__builtin_amdgcn_ballot_w64(t != 0.0f) == 0) return;
#pragma unroll
  for (int c = 0; c < 9; c++) m[c] = material_mix<SDF_EXACT>(m[c], mi[c], t);
}

// One primitive of the owner fold (sdf_abi.h "Queries"): with material_step's
// (a, b) -- the arguments combine hands to min / smin at the running distance
// d and the primitive's value v -- the primitive takes the surface when
// b < a, for a hard and a smooth operator alike (a smooth one blends with
// t = (b < a) ? 1 - q : q, q <= 1/2: the side with the larger weight).  The
// same comparison in both precisions; a tie or a NaN keeps the earlier owner.
__device__ __forceinline__ bool owner_step(int op, float d, float v) {
  const float a = (op == SDF_OP_UNION || op == SDF_OP_SMOOTH_UNION) ? d : -d;
  const float b = (op == SDF_OP_INTERSECT || op == SDF_OP_SMOOTH_INTERSECT) ? -v : v;
  return b < a;
}

// Power-8 Mandelbulb DE, trig-free polynomial form (DESIGN.md Scene spec).
#if SDF_EXACT
// Measured and not kept (profiles/r04_ab_bulb_exact_C5.json, code in git
// history): the map's independent products paired into v_pk_mul_f32
// (+3.7 %), 1/sqrt(k3) without the sqrt guard its proven domain allows
// (+1 %) -- bit-identical, slower (commit 602e5af has them as SDF_BULB_PK /
// _NOGUARD).  max(x2 + z2, 1e-30) as v_max_f32 measured +2 % on the kernel
// of then; on this one C5 exact is 0.1-2.1 % faster with it at three poses,
// with cr_math.h div3_prepared's min3 guard
// (profiles/r06_ab_bulb_min3_k3max.json).
//
// One iteration around its two square roots: bulb_roots forms their
// arguments, bulb_map the rest, given sqrt(m^7) and sqrt(k3).
__device__ __forceinline__ void bulb_roots(const V3& w, float m, float& a7, float& k3) {
  const float m2 = m * m;
  const float m4 = m2 * m2;
  a7 = m4 * m2 * m;
  // v_max_f32: the GLSL select max(x, 1e-30) for x = x^2 + z^2, which is
  // never NaN or -0 (w is finite at the start of an iteration)
  k3 = __builtin_fmaxf(w.x * w.x + w.z * w.z, 1e-30f);
}
__device__ __forceinline__ void bulb_map(const V3& q, V3& w, float& m, float& dz, float s7,
                                         float k3, float sk3) {
  dz = 8.0f * s7 * dz + 1.0f;
  float x = w.x, x2 = x * x, x4 = x2 * x2;
  float y = w.y, y2 = y * y, y4 = y2 * y2;
  float z = w.z, z2 = z * z, z4 = z2 * z2;
  // xz-normalised form of iq's power-8 map (DESIGN.md Scene spec)
  float r = crm::rcp_fast(sk3);   // frsqrt(k3)
  float s = k3 * r;
  float xn = x * r, zn = z * r;
  float xn2 = xn * xn, zn2 = zn * zn, xn4 = xn2 * xn2, zn4 = zn2 * zn2;
  float k1 = x4 + y4 + z4 - 6.0f * y2 * z2 - 6.0f * x2 * y2 + 2.0f * z2 * x2;
  float k4 = x2 - y2 + z2;
  float yk = y * k4 * k1;
  w.x = q.x + 64.0f * yk * xn * zn * (xn2 - zn2) * (xn4 - 6.0f * xn2 * zn2 + zn4) * s;
  w.y = q.y + -16.0f * y2 * k3 * k4 * k4 + k1 * k1;
  w.z = q.z + -8.0f * yk *
                  (xn4 * xn4 - 28.0f * xn4 * xn2 * zn2 + 70.0f * xn4 * zn4 -
                   28.0f * xn2 * zn2 * zn4 + zn4 * zn4) * s;
  m = dot(w, w);
}
// sqrt(k3) keeps cr_sqrt's guard although its domain holds there (k3 in
// [1e-30, 2^65]): without it the kernel measured slower (DESIGN.md
// Appendix A).
__device__ __forceinline__ void bulb_step(const V3& q, V3& w, float& m, float& dz) {
  float a7, k3;
  bulb_roots(w, m, a7, k3);
  const float s7 = fsqrt(a7);
  bulb_map(q, w, m, dz, s7, k3, fsqrt(k3));
}
#else
// The same map with cheaper identities (fast precision: a different rounding
// of the same polynomial; the oracle's own form measured no closer to the
// oracle at 4K and 28 % slower, profiles/r02_bulb_forms.json):
//   |w|^7 = m^3 sqrt(m);  k1 = (x2+z2)^2 + y4 - 6 y2 (x2+z2);  k4 = x2+z2 - y2;
//   (xn + i zn)^8 by three complex squarings: its real part is the w.z
//   polynomial, 8 times its imaginary part the w.x one.
__device__ __forceinline__ void bulb_step(const V3& q, V3& w, float& m, float& dz) {
  dz = fmaf(8.0f * (m * m * m) * fsqrt(m), dz, 1.0f);
  const float x2 = w.x * w.x, y2 = w.y * w.y, z2 = w.z * w.z;
  const float k3 = fmaxf(x2 + z2, 1e-30f);
  const float r = frsqrt(k3);
  const float s = k3 * r;
  float a = w.x * r, b = w.z * r;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float an = fmaf(a, a, -(b * b));
    b = 2.0f * a * b;
    a = an;
  }
  const float k4 = k3 - y2;
  const float k1 = fmaf(k3, fmaf(-6.0f, y2, k3), y2 * y2);
  const float ys = 8.0f * (w.y * k4 * k1) * s;
  w.x = fmaf(ys, b, q.x);
  w.y = q.y + fmaf(k1, k1, -16.0f * y2 * k3 * k4 * k4);
  w.z = fmaf(-ys, a, q.z);
  m = dot(w, w);
}
#endif
// the DE from the orbit's last state
__device__ __forceinline__ float bulb_de(float m, float dz) {
  return fdiv(0.25f * flog(m) * fsqrt(m), dz);
}
__device__ __forceinline__ float mandelbulb(V3 q, int iters, float bail2) {
  V3 w = q;
  float m = dot(w, w);
  float dz = 1.0f;
  for (int i = 0; i < iters; i++) {
    bulb_step(q, w, m, dz);
    if (m > bail2) break;
  }
  return bulb_de(m, dz);
}

// ---- framebuffer formats (sdf_abi.h sdf_format) ----------------------------
// RGBA8 = trunc(min(max(c,0),1) * 255 + 0.5) with NaN -> 0, the multiply and
// add rounded separately (__fmul_rn / __fadd_rn) in both precisions.
__device__ __forceinline__ unsigned to_unorm8(float c) {
  const float q = fminf(fmaxf(c, 0.0f), 1.0f);
  return (unsigned)__fadd_rn(__fmul_rn(q, 255.0f), 0.5f);
}
__device__ __forceinline__ void store_pixel(int format, void* out, size_t o, float4 c) {
  if (format == SDF_FORMAT_RGBA8) {
    const unsigned u = to_unorm8(c.x) | (to_unorm8(c.y) << 8) | (to_unorm8(c.z) << 16) |
                       (to_unorm8(c.w) << 24);
    reinterpret_cast<unsigned*>(out)[o] = u;
  } else if (format == SDF_FORMAT_RGBA16F) {
    const _Float16 h[4] = {(_Float16)c.x, (_Float16)c.y, (_Float16)c.z, (_Float16)c.w};
    uint2 u;
    __builtin_memcpy(&u, h, 8);
    reinterpret_cast<uint2*>(out)[o] = u;
  } else if (format == SDF_FORMAT_RGB32F) {
    float* q = reinterpret_cast<float*>(out) + 3 * o;
    q[0] = c.x;
    q[1] = c.y;
    q[2] = c.z;
  } else {
    reinterpret_cast<float4*>(out)[o] = c;
  }
}

// ---- TILES wire format encoder (sdf_abi.h SDF_FORMAT_TILES) ----------------
// One wave = one 8x8 tile (lane j = pixel 8 * row + column), all 64 lanes
// present; lanes outside the frame carry u = 0 and z = 0.  Neighbours of a
// pixel in the frame are in the frame, so residuals never read those lanes.
// The head goes to its fixed place in the stream, the data to the tile's
// worst-case slot in the scratch area; tiles.hip then compacts the slots into
// the stream in tile order (an allocator shared by every wave would
// serialise on one address).
// Per channel: the gradient residual as the horizontal difference h = u -
// left (DPP row shift; 0 left of the tile) minus the row above's h (one
// ds_bpermute; 0 above the tile), i.e. u - L - U + UL in two neighbour
// reads; zigzag; then one 64 x 64 bit transpose (wave_bits.h) puts plane b
// in lane b and a ballot of the non-zero planes gives the width w (instead
// of a ballot + two v_writelane per plane and a 6-step wave OR).  The base
// width b <= w is the cheapest in bits of w and w - 1 .. w - 12 with an
// escape for the pixels wider than b, all candidates at once in lanes (a
// suffix OR of the planes and a min-reduction: ~30 VALU per channel, where a
// loop of one ballot per candidate spent ~200 mostly scalar instructions and
// 9% of the whole render); the
// escaped pixels' high bits are packed into the tile's bitstream with LDS
// atomic ORs (mbcnt gives each its field index), and so are the base bits,
// pixel by pixel (ABI 10: each lane's low b bits at bit j b; the planes serve
// only the width search, and the decoder loads its bits directly instead of
// transposing: rank 0's N = 8 decode 0.0408 -> 0.0393 ms, the encoder's cost
// unchanged, profiles/r04_lane_major.json).
__device__ __forceinline__ uint32_t ordered_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? (u ^ 0x7fffffffu) : u;
}
// inside each 16-lane DPP row: lane i := OR of lanes i.. (row_shl), max of
// lanes ..i (row_shr); zeros shifted in, so each step is one v_or / v_max
// with a DPP operand
__device__ __forceinline__ uint32_t row_suffix_or(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x101, 0xF, 0xF, true);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x102, 0xF, 0xF, true);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x104, 0xF, 0xF, true);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x108, 0xF, 0xF, true);
  return x;
}
__device__ __forceinline__ uint32_t row_prefix_max(uint32_t x) {
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true));
  return x;
}
__device__ __forceinline__ void store_tiles(void* out, int ntiles, int tile, int lane, bool valid,
                                            float4 c) {
  uint8_t* const base = reinterpret_cast<uint8_t*>(out);
  const int col = lane & 7;
  const TransposeLanes TL(lane);
  const int up = ((lane - 8) & 63) << 2;   // ds_bpermute address of lane - 8
  const int tl = lane & 31;                 // plane index within a half
  const bool low_row = (lane & 16) == 0;    // lanes 0..15, 32..47
  const uint32_t cost0 = 64u * (uint32_t)tl + 72u;
  uint32_t first[3], zc[3];
  int bw[3], wd[3];
  uint64_t esc[3];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const float v = ch == 0 ? c.x : (ch == 1 ? c.y : c.z);
    const uint32_t u = valid ? ordered_bits(v) : 0u;
    // lane - 1 inside the 16-lane DPP row (row_shr:1, 0 shifted in)
    const uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x111, 0xF, 0xF, true);
    const uint32_t h = u - (col ? left : 0u);
    const uint32_t habove = (uint32_t)__builtin_amdgcn_ds_bpermute(up, (int)h);
    const int32_t r = (int32_t)(h - (lane >= 8 ? habove : 0u));   // mod 2^32
    uint32_t zz = ((uint32_t)r << 1) ^ (uint32_t)(r >> 31);      // zigzag
    if (lane == 0 || !valid) zz = 0u;
    first[ch] = __builtin_amdgcn_readfirstlane(u);
    zc[ch] = zz;
  }
  if (__builtin_amdgcn_ballot_w64(((zc[0] | zc[2]) >> 16) != 0u) == 0) {
    // Narrow tile (channels 0 and 2 under 16 bits, most tiles): ONE transpose
    // of (z0 | z2 << 16, z1) -- lanes 0..15 get planes 0..15 of channel 0,
    // 16..31 those of channel 2, 32..63 planes 0..31 of channel 1 -- and one
    // base-width search, each 16-lane DPP row a channel (channel 1 two rows)
    uint32_t a = zc[0] | (zc[2] << 16), b = zc[1];
    transpose64(a, b, TL);
    const uint64_t nz = __builtin_amdgcn_ballot_w64((a | b) != 0u);
    const uint32_t nz0 = (uint32_t)nz & 0xFFFFu, nz2 = (uint32_t)nz >> 16, nz1 = (uint32_t)(nz >> 32);
    wd[0] = nz0 ? 32 - __builtin_clz(nz0) : 0;
    wd[2] = nz2 ? 32 - __builtin_clz(nz2) : 0;
    wd[1] = nz1 ? 32 - __builtin_clz(nz1) : 0;
    const int t = lane < 32 ? (lane & 15) : lane - 32;   // plane of its channel
    const int w = lane < 16 ? wd[0] : (lane < 32 ? wd[2] : wd[1]);
    uint32_t sa = row_suffix_or(a), sb = row_suffix_or(b);
    const uint32_t ra48 = (uint32_t)__builtin_amdgcn_readlane((int)sa, 48);
    const uint32_t rb48 = (uint32_t)__builtin_amdgcn_readlane((int)sb, 48);
    const bool ch1_low = (lane & 48) == 32;   // channel 1's planes 0..15 add 16..31
    sa |= ch1_low ? ra48 : 0u;
    sb |= ch1_low ? rb48 : 0u;
    const uint32_t n = (uint32_t)(__builtin_popcount(sa) + __builtin_popcount(sb));
    const uint32_t cost = 64u * (uint32_t)t + 72u + (uint32_t)(w - t) * n;
    uint32_t nkey = t < w && t >= w - kEscapeWindow ? ~((cost << 6) | (uint32_t)(63 - t)) : 0u;
    nkey = row_prefix_max(nkey);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int pbase = ch == 0 ? 0 : (ch == 2 ? 16 : 32);
      const uint32_t kmax =
          ch == 1 ? max((uint32_t)__builtin_amdgcn_readlane((int)nkey, 47),
                        (uint32_t)__builtin_amdgcn_readlane((int)nkey, 63))
                  : (uint32_t)__builtin_amdgcn_readlane((int)nkey, pbase + 15);
      const uint32_t kmin = ~kmax;
      int bsel = wd[ch];
      uint64_t bmask = 0ull;
      if ((kmin >> 6) < 64u * (uint32_t)wd[ch]) {
        bsel = 63 - (int)(kmin & 63u);
        bmask = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sa, pbase + bsel) |
                (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sb, pbase + bsel) << 32;
      }
      bw[ch] = bsel;
      esc[ch] = bmask;
    }
  } else {
    // Two channels per transpose: lane j holds (z_j of channel A, z_j of B),
    // so lane p < 32 gets plane p of A and lane 32 + p plane p of B (pixels
    // 0..31 in the low word, 32..63 in the high); channel 2 pairs with zeros.
  #pragma unroll
    for (int g = 0; g < 2; g++) {
      const int cA = 2 * g, cB = 2 * g + 1;   // cB = 3: none
      uint32_t a = zc[cA], b = g == 0 ? zc[1] : 0u;
      transpose64(a, b, TL);
      const uint64_t nz = __builtin_amdgcn_ballot_w64((a | b) != 0u);
      const uint32_t nzA = (uint32_t)nz, nzB = (uint32_t)(nz >> 32);
      const int wA = nzA ? 32 - __builtin_clz(nzA) : 0, wB = nzB ? 32 - __builtin_clz(nzB) : 0;
      const int w = lane < 32 ? wA : wB;
      // the cheapest base width: w planes, or t < w planes plus an escape for
      // the n(t) pixels wider than t (their mask, a width byte, w - t bits
      // each), every candidate t in its own lane: the suffix OR of the planes
      // (lanes t.. of the half) is the mask of the pixels wider than t
      // + planes 16..31 of the half (no branch: a readlane inside divergent
      // code may read a lane the branch left undefined)
      uint32_t sa = row_suffix_or(a), sb = row_suffix_or(b);
      const uint32_t ra16 = (uint32_t)__builtin_amdgcn_readlane((int)sa, 16);
      const uint32_t ra48 = (uint32_t)__builtin_amdgcn_readlane((int)sa, 48);
      const uint32_t rb16 = (uint32_t)__builtin_amdgcn_readlane((int)sb, 16);
      const uint32_t rb48 = (uint32_t)__builtin_amdgcn_readlane((int)sb, 48);
      sa |= low_row ? (lane < 32 ? ra16 : ra48) : 0u;
      sb |= low_row ? (lane < 32 ? rb16 : rb48) : 0u;
      const uint32_t n = (uint32_t)(__builtin_popcount(sa) + __builtin_popcount(sb));
      const uint32_t cost = cost0 + (uint32_t)(w - tl) * n;   // 64 t + 72 + (w - t) n
      // candidates t = w - 12 .. w - 1 (t >= 0); the key orders by size, then
      // by the larger t; minimised as its complement (0: no candidate)
      uint32_t nkey = tl < w && tl >= w - kEscapeWindow ? ~((cost << 6) | (uint32_t)(63 - tl)) : 0u;
      nkey = row_prefix_max(nkey);
  #pragma unroll
      for (int hf = 0; hf < 2; hf++) {
        const int ch = hf == 0 ? cA : cB;
        if (ch > 2) break;
        const int wc = hf == 0 ? wA : wB;
        const uint32_t kmin = ~max((uint32_t)__builtin_amdgcn_readlane((int)nkey, 32 * hf + 15),
                                   (uint32_t)__builtin_amdgcn_readlane((int)nkey, 32 * hf + 31));
        int bsel = wc;
        uint64_t bmask = 0ull;
        if ((kmin >> 6) < 64u * (uint32_t)wc) {   // kmin = ~0 (no candidate) never is
          bsel = 63 - (int)(kmin & 63u);
          bmask = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sa, 32 * hf + bsel) |
                  (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sb, 32 * hf + bsel) << 32;
        }
        bw[ch] = bsel;
        wd[ch] = wc;
        esc[ch] = bmask;
      }
    }
  }
  // the escapes' bitstream (width bytes, then each escaped channel's fields
  // in pixel order), assembled in this wave's LDS words
  __shared__ uint32_t escape_bits[kWgWaves][kEscapeDwords];
  uint32_t* const eb = escape_bits[threadIdx.x >> 6];
  const int P = (bw[0] < wd[0]) + (bw[1] < wd[1]) + (bw[2] < wd[2]);
  int nbits = 8 * P;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) nbits += (wd[ch] - bw[ch]) * __builtin_popcountll(esc[ch]);
  const int nbq = (nbits + 63) >> 6;   // bitstream qwords
  if (P) {
    if (lane < 2 * nbq) eb[lane] = 0u;
    if (lane + 64 < 2 * nbq) eb[lane + 64] = 0u;
    // pixel-major fields: this pixel's escaped channels' high bits side by
    // side (channel order), starting after the fields of every lower pixel
    uint32_t widths = 0u, o = 8u * (uint32_t)P;
    uint64_t val = 0ull;
    int nb = 0, j = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      if (bw[ch] == wd[ch]) continue;
      const int d = wd[ch] - bw[ch];
      widths |= (uint32_t)d << (8 * j++);
      const uint64_t m = esc[ch];
      o += (uint32_t)d * __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if ((m >> lane) & 1) {
        val |= (uint64_t)(zc[ch] >> bw[ch]) << nb;   // < 2^d
        nb += d;
      }
    }
    if (nb) {
      const uint32_t s = o & 31, wi = o >> 5;
      atomicOr(&eb[wi], (uint32_t)(val << s));
      if (s + nb > 32) atomicOr(&eb[wi + 1], (uint32_t)((val << s) >> 32));
      if (s + nb > 64) atomicOr(&eb[wi + 2], (uint32_t)(val >> (64 - s)));
    }
    if (lane == 0) atomicOr(&eb[0], widths);
  }
  const int B = bw[0] + bw[1] + bw[2];
  const int nq = B + P + nbq;
  const TilesLayout L(ntiles);
  if (lane == 0)
    reinterpret_cast<uint4*>(base + L.head)[tile] =
        make_uint4((uint32_t)(bw[0] | bw[1] << 6 | bw[2] << 12 | nq << 18 |
                              (bw[0] < wd[0]) << 26 | (bw[1] < wd[1]) << 27 |
                              (bw[2] < wd[2]) << 28),
                   first[0], first[1], first[2]);
  // the tile's data to its slot (tiles.hip compacts the slots): base bits,
  // escape masks, bitstream
  uint2* const q = reinterpret_cast<uint2*>(base + L.slots + (size_t)tile * kTilePlaneBytes);
  // the base bits, lane-major: channel c's bw[c] words follow the earlier
  // channels', pixel j's low bw[c] bits at bit j bw[c] (at most two dwords
  // per pixel), OR-ed into this wave's zeroed LDS words, then stored whole
  __shared__ uint2 base_words[kWgWaves][3 * 32];
  uint2* const bq = base_words[threadIdx.x >> 6];
  uint32_t* const bd = reinterpret_cast<uint32_t*>(bq);
  if (lane < B) bq[lane] = make_uint2(0u, 0u);
  if (lane + 64 < B) bq[lane + 64] = make_uint2(0u, 0u);
  uint32_t qb = 0u;   // the channel's first word
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const int b = bw[ch];
    if (b) {
      const uint32_t v = zc[ch] & (0xFFFFFFFFu >> (32 - b));
      const uint32_t off = 64u * qb + (uint32_t)lane * (uint32_t)b;
      const uint32_t wi = off >> 5, sh = off & 31u;
      atomicOr(&bd[wi], v << sh);
      if (sh + (uint32_t)b > 32u) atomicOr(&bd[wi + 1], v >> (32u - sh));
    }
    qb += (uint32_t)b;
  }
  if (lane < B) q[lane] = bq[lane];
  if (lane + 64 < B) q[lane + 64] = bq[lane + 64];
  int k = bw[0] + bw[1] + bw[2];
  if (lane == 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
      if (bw[ch] < wd[ch]) q[k++] = make_uint2((uint32_t)esc[ch], (uint32_t)(esc[ch] >> 32));
  }
  if (P) {
    uint32_t* const bits = reinterpret_cast<uint32_t*>(q + B + P);
    if (lane < 2 * nbq) bits[lane] = eb[lane];
    if (lane + 64 < 2 * nbq) bits[lane + 64] = eb[lane + 64];
  }
}
// Stream header words 2..15 (sdf_abi.h SDF_FORMAT_TILES): what the channels
// hold and the frame's shading constants, written by tile 0's wave (words 0
// and 1 are tiles_move's)
__device__ __forceinline__ void store_tiles_shade(void* out, const ShadeK& K, int lane) {
  if (lane >= 14) return;
  const float k[10] = {K.lam[0], K.lam[1], K.lam[2], K.dif[0], K.dif[1],
                       K.dif[2], K.ref[0], K.ref[1], K.ref[2], K.shin};
  uint32_t v = 0u;
  if (lane == 0) v = SDF_EXACT ? kTilesShadeExact : kTilesShadeFast;
#pragma unroll
  for (int i = 0; i < 10; i++)
    if (lane == 2 + i) v = __float_as_uint(k[i]);
  reinterpret_cast<uint32_t*>(out)[2 + lane] = v;
}

// ---- scene evaluators -------------------------------------------------------
// sceneSDF, voxel_fragment.frag:73-81: d = INF, one combine per primitive.

// Per-lane state a scene may carry along one march (see FixedScene::march):
// cached bound gaps (+ the ray distance of their test) of the cluster and of
// up to kMaxCached primitives.
constexpr int kMaxCached = 8;
struct MarchState {
  float gt = -INFINITY;
  float gu = INFINITY;   // cluster gap upper bound: g_c - t_c (see FixedScene::march)
  float pg[kMaxCached];
#ifdef SDF_STATS
  int stage = 0;   // 0 primary ray, 1 normal / AO probes, 2 shadow ray
#endif
  __device__ __forceinline__ MarchState() {
#pragma unroll
    for (int i = 0; i < kMaxCached; i++) pg[i] = -INFINITY;
  }
};

// Debug instrumentation (tools/kernel_stats.py; a separate library built with
// -DSDF_STATS): wave-level event counts per pipeline stage.  Events: 0 scene
// evaluations, 1 cluster skipped on its cached gap, 2 cluster fresh test,
// 3 cluster skipped after its fresh test, 4+i primitive i skipped on its cached
// gap, 12+i primitive i fresh test, 20+i primitive i evaluated.
#ifdef SDF_STATS
__device__ unsigned long long g_sdf_stats[128];
__device__ __forceinline__ void sdf_stat(int i) {
  const unsigned long long ex = __builtin_amdgcn_read_exec();
  if ((int)(threadIdx.x & 63) == __builtin_ctzll(ex)) atomicAdd(&g_sdf_stats[i], 1ull);
}
#define STAT(st, e) sdf_stat((st).stage * 32 + (e))
#else
#define STAT(st, e) ((void)0)
#endif

// true when some active lane is within the bound (c, K') and must evaluate
// (kernel_args.h "exact bounding-volume culling").  A lane is far when
// |p - c| >= T = (d + K) / (1 - kCullRel) = d*kCullScale + K' (K' prepared on
// the host); dd >= T*T tests that for T >= 0, and for T < 0 it is either true
// (skip, valid since |p - c| >= 0 > T) or false (evaluate, always valid).  A
// NaN T evaluates.  Branch-free per lane, one wave-uniform answer.
// |p - c|^2 of a culling test.  Its rounding is covered by the tests'
// margins (kCullRel), so exact precision may fuse it (FUSE: two FMAs, two
// VALU fewer per test); a sphere's own bound keeps the plain sum, which its
// SDF computes too (one computation for both).  Fast precision contracts
// either form by itself.
template <bool FUSE>
__device__ __forceinline__ float cull_dist2(float dx, float dy, float dz) {
  if constexpr (FUSE && SDF_EXACT)
    return __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
  else
    return dx * dx + dy * dy + dz * dz;
}

template <bool FUSE = true>
__device__ __forceinline__ bool wave_near(float cx, float cy, float cz, float K, V3 p, float d) {
  const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
  const float dd = cull_dist2<FUSE>(dx, dy, dz);
  const float T = __builtin_fmaf(d, kCullScale, K);
  return __builtin_amdgcn_ballot_w64(!(dd >= T * T)) != 0;
}

// The normal's taps around P, generated on demand (no VGPRs held per tap).
// Tetrahedral (DESIGN.md Scene spec): P + h e_j, e_0 = (1,-1,-1),
// e_1 = (-1,-1,1), e_2 = (-1,1,-1), e_3 = (1,1,1); |h| sqrt 3 from P.
struct TetraTaps {
  static constexpr int K = 4;
  V3 P;
  float h;
  __device__ __forceinline__ V3 operator()(int j) const {
    switch (j) {
      case 0: return mk(P.x + h, P.y - h, P.z - h);
      case 1: return mk(P.x - h, P.y - h, P.z + h);
      case 2: return mk(P.x - h, P.y + h, P.z - h);
      default: return mk(P.x + h, P.y + h, P.z + h);
    }
  }
};
// Central differences, voxel_fragment.frag:134-155: P -/+ h along x, y, z
// (taps 2a, 2a + 1 on axis a); |h| from P.
struct CentralTaps {
  static constexpr int K = 6;
  V3 P;
  float h;
  __device__ __forceinline__ V3 operator()(int j) const {
    switch (j) {
      case 0: return mk(P.x - h, P.y, P.z);
      case 1: return mk(P.x + h, P.y, P.z);
      case 2: return mk(P.x, P.y - h, P.z);
      case 3: return mk(P.x, P.y + h, P.z);
      case 4: return mk(P.x, P.y, P.z - h);
      default: return mk(P.x, P.y, P.z + h);
    }
  }
};

// The default 5 AO taps P + N h_i as one batch (FixedScene::taps): each
// lies within |h_i| <= ao_path[4] of P (host, rounded up).
struct AOTaps {
  static constexpr int K = 5;
  V3 P, N;
  KF h;
  __device__ __forceinline__ V3 operator()(int j) const { return add(P, muls(N, h[j])); }
};

// Any primitive list: kinds and ops are read (scalar loads, uniform branches)
// at every evaluation.  The cullable suffix [cluster_first, count) is culled
// exactly like the fixed scenes' (one cluster bound, then one bound per
// primitive), without the cached gaps; cluster_first = count (dispatch
// SDF_DISPATCH_UNCULLED) evaluates every primitive everywhere.
struct GenericScene {
  KA& A;
  static constexpr bool kBatchedTaps = false;
  static constexpr bool kPlaneHead = false;
  __device__ __forceinline__ explicit GenericScene(KA& a) : A(a) {}
  __device__ __forceinline__ float march(V3 p, float, MarchState&) const { return eval(p); }
  __device__ __forceinline__ float march_primary(V3 p, float, MarchState&) const { return eval(p); }
  __device__ __forceinline__ float eval(V3 p) const {
    float d = INFINITY;  // INF, :20, :75
    const int n = A.prim_count;
    const int cf = A.cluster_first < n ? A.cluster_first : n;
    for (int i = 0; i < cf; i++) {
      const KARG sdf_primitive& pr = A.prims[i];
      KF q = pr.p;
      d = combine(pr.op, d, prim_sdf(pr.kind, p, q), SMIN_K(pr), SMIN_IK(pr), SMIN_SC(pr),
                    SMIN_KSC(pr));
    }
    if (cf < n && wave_near(A.cluster[0], A.cluster[1], A.cluster[2], A.cluster[3], p, d)) {
      for (int i = cf; i < n; i++) {
        KF bd = A.bound[i];
        if (!wave_near(bd[0], bd[1], bd[2], bd[3], p, d)) continue;
        const KARG sdf_primitive& pr = A.prims[i];
        KF q = pr.p;
        d = combine(pr.op, d, prim_sdf(pr.kind, p, q), SMIN_K(pr), SMIN_IK(pr), SMIN_SC(pr),
                    SMIN_KSC(pr));
      }
    }
    return d;
  }
  // the material fold at p (material_step): every primitive, unculled, in
  // list order, d advanced as eval does
  __device__ __forceinline__ void material_fold(V3 p, const KARG MaterialArgs& M,
                                                float (&m)[9]) const {
    float d = INFINITY;
    const int n = A.prim_count;
    for (int i = 0; i < n; i++) {
      const KARG sdf_primitive& pr = A.prims[i];
      KF q = pr.p;
      const float v = prim_sdf(pr.kind, p, q);
      material_step(pr.op, d, v, SMIN_K(pr), SMIN_IK(pr), M.m[i], m);
      d = combine(pr.op, d, v, SMIN_K(pr), SMIN_IK(pr), SMIN_SC(pr), SMIN_KSC(pr));
    }
  }
  // the owner fold at p (owner_step): every primitive, unculled, in list
  // order, d advanced as eval does; the index of the primitive that owns p
  __device__ __forceinline__ int owner_fold(V3 p) const {
    float d = INFINITY;
    int w = 0;
    const int n = A.prim_count;
    for (int i = 0; i < n; i++) {
      const KARG sdf_primitive& pr = A.prims[i];
      KF q = pr.p;
      const float v = prim_sdf(pr.kind, p, q);
      if (owner_step(pr.op, d, v)) w = i;
      d = combine(pr.op, d, v, SMIN_K(pr), SMIN_IK(pr), SMIN_SC(pr), SMIN_KSC(pr));
    }
    return w;
  }
};

// kinds whose value is never -0 (smin<HW>)
constexpr bool no_neg_zero(int kind) { return kind != SDF_PRIM_PLANE && kind != kPrimPlaneY; }

template <int KIND, class Q>
__device__ __forceinline__ float prim_ct(V3 p, const Q& q) {
  if constexpr (KIND == SDF_PRIM_SPHERE) return sd_sphere(p, q);
  else if constexpr (KIND == SDF_PRIM_PLANE) return sd_plane(p, q);
  else if constexpr (KIND == kPrimPlaneY) return p.y + q[3];  // planeSDF :68 (n = +y)
  else if constexpr (KIND == SDF_PRIM_BOX) return sd_box(p, q);
  else if constexpr (KIND == SDF_PRIM_ROUND_BOX) return sd_round_box(p, q);
  else if constexpr (KIND == SDF_PRIM_TORUS) return sd_torus(p, q);
  else if constexpr (KIND == SDF_PRIM_CAPSULE) return sd_capsule(p, q);
  else return sd_cylinder(p, q);
}

// A primitive list whose kinds and ops are fixed at compile time.  The
// parameter values are runtime uniforms, loaded once per wave into registers
// (SGPRs) before the march loops: no per-evaluation branching or reloads.
//
// Exact culling (kernel_args.h): the cullable suffix of the list sits behind
// one cluster bound and each of its primitives behind its own bound; a test
// skips work only when every active lane of the wave passes it (wave-uniform
// branch), and a skipped primitive would have left d unchanged bit for bit,
// so results and step counts equal the unculled evaluation.
template <int... KO>
struct FixedScene {
  static constexpr int N = sizeof...(KO);
  static constexpr int kKO[N] = {KO...};
  static constexpr int first_culled() {
    int f = N;
    while (f > 0 && cullable(kKO[f - 1] >> 3, kKO[f - 1] & 7)) --f;
    return f;
  }
  static constexpr int kFirst = first_culled();
  static constexpr bool kBatchedTaps = true;
  float q[N][9];
  float k[N], ik[N], sc[N], ksc[N];
  float kg[N];   // exact, cullable primitives: the own-value gap's offset (step_cached)
  float b[N][4];  // bound: centre (read only for capsules; the others use q[i][0..2]), K
  float cl[4];
  __device__ __forceinline__ explicit FixedScene(KA& A) {
#pragma unroll
    for (int i = 0; i < N; i++) {
#pragma unroll
      for (int j = 0; j < 9; j++) q[i][j] = A.prims[i].p[j];
      k[i] = SMIN_K(A.prims[i]);
      ik[i] = SMIN_IK(A.prims[i]);
      sc[i] = SMIN_SC(A.prims[i]);
      // k sc is the smooth-min FMA's third operand beside the SGPR sc (one
      // SGPR per VALU on gfx950): held in a VGPR for the wave, once, instead
      // of a v_mov at every evaluation
      const int op = kKO[i] & 7;
      const bool smooth = op == SDF_OP_SMOOTH_UNION || op == SDF_OP_SMOOTH_SUBTRACT ||
                          op == SDF_OP_SMOOTH_INTERSECT;
      ksc[i] = (SDF_EXACT && smooth) ? to_vgpr(SMIN_KSC(A.prims[i])) : SMIN_KSC(A.prims[i]);
      kg[i] = A.prims[i].reserved;
    }
    // bounds are read rarely (cached gaps): VGPRs, loaded as float4 vectors
    // (exact precision, kBoundsInVgprs false: uniform kernel-argument values,
    // which the compiler keeps in SGPRs or reloads with scalar loads)
    const int vz = kBoundsInVgprs ? lane_zero() : 0;
#pragma unroll
    for (int i = kFirst; i < N; i++) {
#pragma unroll
      for (int j = 0; j < 4; j++) b[i][j] = (&A.bound[0][0])[(i + vz) * 4 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) cl[j] = A.cluster[vz * 4 + j];
  }
  // d combined with the primitive value v
  template <int I>
  __device__ __forceinline__ float apply(float d, float v) const {
    constexpr int ko = kKO[I];
    return combine<no_neg_zero(ko >> 3)>(ko & 7, d, v, k[I], ik[I], sc[I], ksc[I]);
  }
  template <int I>
  __device__ __forceinline__ float step(float d, V3 p) const {
    constexpr int ko = kKO[I];
    if constexpr (I >= kFirst) {
      const bool cap = (ko >> 3) == SDF_PRIM_CAPSULE;
      const float cx = cap ? b[I][0] : q[I][0];
      const float cy = cap ? b[I][1] : q[I][1];
      const float cz = cap ? b[I][2] : q[I][2];
      if (!wave_near<(ko >> 3) != SDF_PRIM_SPHERE>(cx, cy, cz, b[I][3], p, d)) return d;
    }
    return apply<I>(d, prim_ct<(ko >> 3)>(p, q[I]));
  }
  template <int... I>
  __device__ __forceinline__ float prefix(float d, V3 p, Seq<I...>) const {
    ((d = I < kFirst ? step<I>(d, p) : d), ...);
    return d;
  }
  // the accumulator before the cullable suffix, from d = INF (:75)
  __device__ __forceinline__ float head(V3 p) const {
    // min(INF, v) = v for every non-NaN v: start from the first primitive.
    // Exact precision too: the GLSL select min(INF, v) differs only for a
    // NaN v, and sdf_validate's working range keeps every primitive value
    // finite
    if constexpr (kFirst > 0 && (kKO[0] & 7) == SDF_OP_UNION)
      return prefix(prim_ct<(kKO[0] >> 3)>(p, q[0]), p, MakeSeq<N>{}, 1);
    return prefix(INFINITY, p, MakeSeq<N>{});
  }
  template <int... I>
  __device__ __forceinline__ float prefix(float d, V3 p, Seq<I...>, int) const {
    ((d = (I >= 1 && I < kFirst) ? step<I>(d, p) : d), ...);
    return d;
  }
  template <int... I>
  __device__ __forceinline__ float suffix(float d, V3 p, Seq<I...>) const {
    ((d = I >= kFirst ? step<I>(d, p) : d), ...);
    return d;
  }
  // step<I> with the primitive's bound gap cached along the march (see march)
  // (dt = d + t: the cached test pg - t >= d as pg >= dt, one compare per
  // primitive, refreshed when a primitive changes d).  A fresh test is the
  // cached test of the gap it has just stored (pg >= dt, the same comparison
  // at t - t_c = 0, so valid by the same margins) instead of g >= d / (1 -
  // kCullRel): no second accumulator d / (1 - kCullRel) to keep (one multiply
  // fewer per evaluated primitive and per visit of the suffix).  Exact
  // precision: an evaluated primitive's cached gap comes from its own value
  // instead of its bounding sphere.
  template <int I>
  __device__ __forceinline__ float step_cached(float d, V3 p, float t, float& dt,
                                               MarchState& st) const {
    constexpr int ko = kKO[I];
    constexpr int slot = I - kFirst;
    if constexpr (I >= kFirst && slot < kMaxCached) {
      if (__builtin_amdgcn_ballot_w64(!(st.pg[slot] >= dt)) == 0) {
        STAT(st, 4 + slot);
        return d;
      }
      STAT(st, 12 + slot);
      const bool cap = (ko >> 3) == SDF_PRIM_CAPSULE;
      const float dx = p.x - (cap ? b[I][0] : q[I][0]);
      const float dy = p.y - (cap ? b[I][1] : q[I][1]);
      const float dz = p.z - (cap ? b[I][2] : q[I][2]);
      const float g =
          __builtin_amdgcn_sqrtf(cull_dist2<(ko >> 3) != SDF_PRIM_SPHERE>(dx, dy, dz)) - b[I][3];
      st.pg[slot] = fmaf(g, 1.0f - kCullRel, t);
      if (__builtin_amdgcn_ballot_w64(!(st.pg[slot] >= dt)) == 0) return d;
      STAT(st, 20 + slot);
      const float v = prim_ct<(ko >> 3)>(p, q[I]);
      d = apply<I>(d, v);
#if SDF_EXACT
      // the evaluated primitive's own value bounds its values along the rest
      // of the path (an exact SDF is 1-Lipschitz): its gap v - (k + margin)
      // replaces the bounding sphere's, which is never larger.  The margin
      // (host, prims[].reserved) adds 1e-4 R to kCullAbs, covering the fp32
      // error of v, which is relative to the magnitudes v is formed from
      // (|p - c| <= R + |v| where it matters), beside the relative 1e-5
      st.pg[slot] = fmaf(v - kg[I], 1.0f - kCullRel, t);
#endif
      dt = d + t;
      return d;
    } else {
      d = step<I>(d, p);
      dt = d + t;
      return d;
    }
  }
  template <int... I>
  __device__ __forceinline__ float suffix_cached(float d, V3 p, float t, float dt, MarchState& st,
                                                 Seq<I...>) const {
    ((d = I >= kFirst ? step_cached<I>(d, p, t, dt, st) : d), ...);
    return d;
  }
  __device__ __forceinline__ float eval(V3 p) const {
    float d = head(p);
    if constexpr (kFirst < N) {
      if (wave_near(cl[0], cl[1], cl[2], cl[3], p, d)) d = suffix(d, p, MakeSeq<N>{});
    }
    return d;
  }
  // The material fold at p (material_step), unrolled over the list: every
  // primitive, unculled, with its compile-time kind and operator, d advanced
  // by the march's own combine (apply), so it holds the bits it has there.
  template <int I>
  __device__ __forceinline__ void material_fold_step(float& d, V3 p, const KARG MaterialArgs& M,
                                                     float (&m)[9]) const {
    constexpr int ko = kKO[I];
    const float v = prim_ct<(ko >> 3)>(p, q[I]);
    material_step(ko & 7, d, v, k[I], ik[I], M.m[I], m);
    d = apply<I>(d, v);
  }
  template <int... I>
  __device__ __forceinline__ void material_fold_seq(V3 p, const KARG MaterialArgs& M,
                                                    float (&m)[9], Seq<I...>) const {
    float d = INFINITY;
    (material_fold_step<I>(d, p, M, m), ...);
  }
  __device__ __forceinline__ void material_fold(V3 p, const KARG MaterialArgs& M,
                                                float (&m)[9]) const {
    material_fold_seq(p, M, m, MakeSeq<N>{});
  }
  // The owner fold at p (owner_step), unrolled like the material fold: every
  // primitive, unculled, d advanced by the march's own combine (apply).
  template <int I>
  __device__ __forceinline__ void owner_fold_step(float& d, int& w, V3 p) const {
    constexpr int ko = kKO[I];
    const float v = prim_ct<(ko >> 3)>(p, q[I]);
    if (owner_step(ko & 7, d, v)) w = I;
    d = apply<I>(d, v);
  }
  template <int... I>
  __device__ __forceinline__ int owner_fold_seq(V3 p, Seq<I...>) const {
    float d = INFINITY;
    int w = 0;
    (owner_fold_step<I>(d, w, p), ...);
    return w;
  }
  __device__ __forceinline__ int owner_fold(V3 p) const { return owner_fold_seq(p, MakeSeq<N>{}); }
  // Evaluation at a point p reached by a path of length t (see the pixel
  // pipeline: the primary ray, then side trips to the normal / AO taps and the
  // shadow ray).  Bounds are cached along the path: a fresh test at path
  // length t_c finds the lane's gap g = (|p - C| - K') (1 - kCullRel) (the
  // cluster, and each primitive of the cullable suffix); at path length t the
  // gap is still at least g - (t - t_c) (triangle inequality; t carries a
  // kPathScale factor against rounding of unit directions), so while
  // g - (t - t_c) >= d for every active lane the test is skipped.  The state
  // holds g + t_c (-inf before the first test).  Same skips, same results.
  //
  // The cluster also keeps an upper bound: its gap is at most g + (t - t_c).
  // When that is below d on some lane, the wave's fresh cluster test cannot
  // pass (typically a path inside the cluster sphere), so it is not made and
  // the primitives are tested directly.  This only ever forgoes a skip, so it
  // needs no rounding margin.
  //
  // The cluster's cached test is gt >= dt, dt = d + t -- the primitives' form
  // (pg >= dt), with dt then handed to them instead of being formed again.
  __device__ __forceinline__ float march(V3 p, float t, MarchState& st) const {
    return march_at<false>(p, t, st);
  }
  // the primary ray's evaluation at ray distance r (path length r kPathScale):
  // forms dt = d + r kPathScale with one FMA, and the path length itself only
  // where a gap is stored (the cached tests need only dt): C4 exact 0.3-0.4 %
  // faster at three poses, bit-identical (profiles/r06_ab_dtfma_evalskip.json)
  __device__ __forceinline__ float march_primary(V3 p, float r, MarchState& st) const {
    return march_at<true>(p, r, st);
  }
  template <bool LIN>
  __device__ __forceinline__ float march_at(V3 p, float tr, MarchState& st) const {
    float d = head(p);
    STAT(st, 0);
    if constexpr (kFirst < N) {
      const float t = LIN ? tr * kPathScale : tr;
      const float dt = LIN ? fmaf(tr, kPathScale, d) : d + t;
      if (__builtin_amdgcn_ballot_w64(!(st.gt >= dt)) != 0) {
        if (__builtin_amdgcn_ballot_w64(st.gu + t < d) == 0) {
          STAT(st, 2);
          const float dx = p.x - cl[0], dy = p.y - cl[1], dz = p.z - cl[2];
          const float g =
              (__builtin_amdgcn_sqrtf(cull_dist2<true>(dx, dy, dz)) - cl[3]) * (1.0f - kCullRel);
          st.gt = g + t;
          st.gu = g - t;
          if (__builtin_amdgcn_ballot_w64(!(g >= d)) == 0) {
            STAT(st, 3);
            return d;
          }
        } else {
          STAT(st, 28);
        }
        d = suffix_cached(d, p, t, dt, st, MakeSeq<N>{});
      } else {
        STAT(st, 1);
      }
    }
    return d;
  }

  // The normal's taps (TetraTaps: 4, CentralTaps: 6) with ONE culling
  // decision per bound for all of them.  The taps lie within a distance r of
  // P (|h| sqrt 3, |h|), which is on the pixel's path at path length tP, so a
  // bound's gap measured AT P (recorded in the path state: the AO taps and
  // the shadow ray that follow start from P too) bounds the gap at every tap
  // reached with path length tt = tP + r (kPathScale): the cached-gap test of
  // march() against dm = the largest of the taps' accumulators.  A skip
  // therefore leaves every tap's accumulator unchanged bit for bit (same
  // margins as march()); a bound that does not pass evaluates its primitive
  // at every tap.  Instead of one cluster test, one cached test and up to one
  // fresh test per primitive for EACH tap: one of each.
  template <class T>
  static __device__ __forceinline__ float max_of(const float (&f)[T::K]) {
    float m = fmaxf(f[0], f[1]);
#pragma unroll
    for (int j = 2; j < T::K; j++) m = fmaxf(m, f[j]);
    return m;
  }
  template <int I, class T>
  __device__ __forceinline__ void taps_step(float (&f)[T::K], const T& tap, float tP, float tt,
                                            float& dt, MarchState& st) const {
    constexpr int ko = kKO[I];
    constexpr int slot = I - kFirst;
    const V3 P = tap.P;
    if constexpr (I >= kFirst && slot < kMaxCached) {
      if (__builtin_amdgcn_ballot_w64(!(st.pg[slot] >= dt)) == 0) {
        STAT(st, 4 + slot);
        return;
      }
      STAT(st, 12 + slot);
      const bool cap = (ko >> 3) == SDF_PRIM_CAPSULE;
      const float dx = P.x - (cap ? b[I][0] : q[I][0]);
      const float dy = P.y - (cap ? b[I][1] : q[I][1]);
      const float dz = P.z - (cap ? b[I][2] : q[I][2]);
      const float g = __builtin_amdgcn_sqrtf(cull_dist2<true>(dx, dy, dz)) - b[I][3];
      st.pg[slot] = fmaf(g, 1.0f - kCullRel, tP);
      if (__builtin_amdgcn_ballot_w64(!(st.pg[slot] >= dt)) == 0) return;
    }
    if constexpr (I >= kFirst) {
      if constexpr (slot < kMaxCached) STAT(st, 20 + slot);
#pragma unroll
      for (int j = 0; j < T::K; j++) f[j] = apply<I>(f[j], prim_ct<(ko >> 3)>(tap(j), q[I]));
      dt = max_of<T>(f) + tt;
    }
  }
  template <class T, int... I>
  __device__ __forceinline__ void taps_suffix(float (&f)[T::K], const T& tap, float tP, float tt,
                                              MarchState& st, Seq<I...>) const {
    float dt = max_of<T>(f) + tt;
    (taps_step<I>(f, tap, tP, tt, dt, st), ...);
  }
  template <class T>
  __device__ __forceinline__ void taps(const T& tap, float tP, float tt, MarchState& st,
                                       float (&f)[T::K]) const {
#ifdef SDF_STATS
    st.stage = 1;   // counted with the probes (one event per batch of taps)
#endif
#pragma unroll
    for (int j = 0; j < T::K; j++) f[j] = head(tap(j));
    STAT(st, 0);
    if constexpr (kFirst < N) {
      const float dm = max_of<T>(f);
      if (__builtin_amdgcn_ballot_w64(!(st.gt - tt >= dm)) == 0) {
        STAT(st, 1);
        return;
      }
      STAT(st, 2);
      const V3 P = tap.P;
      const float dx = P.x - cl[0], dy = P.y - cl[1], dz = P.z - cl[2];
      const float g =
          (__builtin_amdgcn_sqrtf(cull_dist2<true>(dx, dy, dz)) - cl[3]) * (1.0f - kCullRel);
      st.gt = g + tP;
      st.gu = g - tP;
      if (__builtin_amdgcn_ballot_w64(!(st.gt - tt >= dm)) == 0) {
        STAT(st, 3);
        return;
      }
      taps_suffix(f, tap, tP, tt, st, MakeSeq<N>{});
    }
  }

  // ---- the shadow march's lit tail (render path without step counts) ----
  // The head is one plane and the rest of the list lies in the cluster
  // sphere (C, K').  Along the shadow ray o + L t the plane is h(t) = a + b t.
  // Wherever (|o + L t - C| - K')(1 - kCullRel) >= h(t) -- the cluster
  // culling's own sufficient condition for an unchanged accumulator -- the
  // scene value IS the plane's.  f(t) = that difference is convex in t, so
  // once f(ts) >= 0 and f'(ts) >= 0 it holds at every later point: from the
  // first step taken at t >= ts on, the march is h_n = (1 + b) h_(n-1),
  // t_n = (h_n - a) / b, and voxel_fragment.frag:105-132's terms
  // k sqrt(h^2 - y^2) / (t - y), y = h^2 / (2 h_(n-1)), equal
  // k sqrt(1 - r^2/4) h / (h c - a/b) (r = 1 + b, c = 1/b - r/2 > 0 for
  // b < 1): for a > 0 they decrease with h towards
  //   lim = k b sqrt(1 - r^2/4) / (1 - b r / 2)
  // (a non-positive denominator gives +INF).  With lim >= 1 no later term
  // can change clamp(s, 0, 1) -- min(s, term) is s when s <= 1 and clamps to
  // 1 otherwise -- so the march may end there, bit for bit the same shadow.
  // Returns the limit for the march's `t > limit` break: a step taken at
  // t_c ends at t <= t_c + h(t_c) = a + (1 + b) t_c (the scene never exceeds
  // its head), so t > a + (1 + b) ts proves t_c >= ts.  `lit`: ts = 0, the
  // whole march leaves s = 1 (its first term is +INF).  Margins: lim >= 1.01,
  // b <= 0.95 (lim's sensitivity to the fp32 ratio stays small), ts moved
  // out by 1e-3 (1 + ts), f and f' checked with 1e-4 (1 + ts + |p - C|).
  static constexpr bool kPlaneHead =
      kFirst == 1 && kFirst < N && (kKO[0] & 7) == SDF_OP_UNION &&
      ((kKO[0] >> 3) == kPrimPlaneY || (kKO[0] >> 3) == SDF_PRIM_PLANE);
  // the head plane along o + L t: value a at t = 0, slope b
  __device__ __forceinline__ void plane_line(V3 o, V3 L, float& a, float& b) const {
    if constexpr ((kKO[0] >> 3) == kPrimPlaneY) {
      a = o.y + q[0][3];
      b = L.y;
    } else {
      a = sd_plane(o, q[0]);
      b = dot(L, mk(q[0][0], q[0][1], q[0][2]));
    }
  }
  // The smallest ts >= 0 (margins included) past which the ray o + L t
  // (|L| = 1) is plane-only: f(t) = (|o + L t - C| - K')(1 - kCullRel) -
  // (a + b t) >= 0 for every t >= ts; +INF when that is not proved (|b| >
  // 0.95 or `ok` false).  f is convex, so f(ts) >= 0 and f'(ts) >= 0 prove it
  // for every later t; ts is proposed as the larger root of
  // |w + L t|^2 = (alpha + beta t)^2, w = o - C, and verified in fp32 with a
  // margin of 1e-4 (1 + ts + |p - C|), after moving it out by 1e-3 (1 + ts).
  __device__ __forceinline__ float plane_clear(V3 o, V3 L, float a, float b, bool ok) const {
    ok = ok && fabsf(b) <= 0.95f;
    if (__builtin_amdgcn_ballot_w64(ok) == 0) return INFINITY;
    const float wx = o.x - cl[0], wy = o.y - cl[1], wz = o.z - cl[2];
    const float m = wx * L.x + wy * L.y + wz * L.z;
    const float ww = wx * wx + wy * wy + wz * wz;
    const float beta = b * kCullScale, alpha = fmaf(a, kCullScale, cl[3]);
    const float qa = fmaf(-beta, beta, 1.0f);
    const float qb = fmaf(-alpha, beta, m);
    const float qc = fmaf(-alpha, alpha, ww);
    const float disc = fmaf(qb, qb, -qa * qc);
    float ts = disc > 0.0f ? (__builtin_amdgcn_sqrtf(disc) - qb) * __builtin_amdgcn_rcpf(qa) : 0.0f;
    ts = ts > 0.0f ? fmaf(ts, 1.001f, 1e-3f) : 0.0f;
    const float px = fmaf(L.x, ts, wx), py = fmaf(L.y, ts, wy), pz = fmaf(L.z, ts, wz);
    const float dist = __builtin_amdgcn_sqrtf(px * px + py * py + pz * pz);
    const float margin = 1e-4f * (1.0f + ts + dist);
    const bool holds = ok && (dist - cl[3]) * (1.0f - kCullRel) - fmaf(b, ts, a) >= margin &&
                       (m + ts) * (1.0f - kCullRel) >= fmaf(b, dist, margin);
    return holds ? ts : INFINITY;
  }
  __device__ __forceinline__ float shadow_limit(V3 o, V3 L, float k, float tmax,
                                                bool& lit) const {
    float a, b;
    plane_line(o, L, a, b);
    const float r = 1.0f + b;
    const float lim = k * b * __builtin_amdgcn_sqrtf(fmaxf(1.0f - 0.25f * r * r, 0.0f)) *
                      __builtin_amdgcn_rcpf(1.0f - 0.5f * b * r);
    const float ts = plane_clear(o, L, a, b, a > 0.0f && b > 0.0f && lim >= 1.01f);
    lit = ts == 0.0f;
    return ts == INFINITY ? tmax : fminf(tmax, fmaf(r, ts, a) * 1.00001f);
  }
};

// A side trip from the path (normal and AO taps): uses the cached gaps with
// the tap's path length but records nothing, so later queries along the main
// path stay valid.
template <class Scene>
__device__ __forceinline__ float probe(const Scene& scene, V3 p, float t, MarchState st) {
#ifdef SDF_STATS
  st.stage = 1;
#endif
  return scene.march(p, t, st);
}

// The normal's taps: batched culling (FixedScene::taps) or one probe each.
template <class Scene, class T>
__device__ __forceinline__ void normal_taps(const Scene& scene, const T& tap, float tP, float tt,
                                            MarchState& st, float (&f)[T::K]) {
  if constexpr (Scene::kBatchedTaps) {
    scene.taps(tap, tP, tt, st, f);
  } else {
    (void)tP;
#pragma unroll
    for (int j = 0; j < T::K; j++) f[j] = probe(scene, tap(j), tt, st);
  }
}

// The Mandelbulb's normal and AO taps go one after another (scene.march per
// tap): lockstep groups of orbits measured slower (DESIGN.md Appendix A).
struct BulbScene {
  static constexpr bool kBatchedTaps = false;
  static constexpr bool kPlaneHead = false;
  float c0, c1, c2, sc, isc, bail2;
  int iters;
  __device__ __forceinline__ explicit BulbScene(KA& A)
      : c0(A.bulb_center[0]), c1(A.bulb_center[1]), c2(A.bulb_center[2]), sc(A.bulb_scale),
        isc(A.bulb_inv_scale), bail2(A.bulb_bail2), iters(A.bulb_iterations) {}
  __device__ __forceinline__ float march(V3 p, float, MarchState&) const { return eval(p); }
  __device__ __forceinline__ float march_primary(V3 p, float, MarchState&) const { return eval(p); }
  __device__ __forceinline__ V3 local(V3 p) const {
#if SDF_EXACT
    // (p - c) / scale by Markstein's steps from the host's RN(1/scale), for a
    // scale in [2^-30, 2^30) (a wave-uniform test; the IEEE division else)
    float a0 = p.x - c0, a1 = p.y - c1, a2 = p.z - c2;
    if (crm::divisor_ok(sc)) {
      crm::div3_prepared(a0, a1, a2, sc, isc);
      return mk(a0, a1, a2);
    }
    return mk(a0 / sc, a1 / sc, a2 / sc);
#else
    return mk((p.x - c0) * isc, (p.y - c1) * isc, (p.z - c2) * isc);
#endif
  }
  __device__ __forceinline__ float eval(V3 p) const {
    V3 q = local(p);
    // bounding sphere |q| = 1.5: the set lies within 1.25 (DESIGN.md)
    float m0 = dot(q, q);
    if (m0 > 2.25f) return (fsqrt(m0) - 1.25f) * sc;
    return mandelbulb(q, iters, bail2) * sc;
  }
  // the one shape owns every point (sdf_abi.h "Queries")
  __device__ __forceinline__ int owner_fold(V3) const { return 0; }
};

#define scene_sdf(A, p) scene.eval(p)

// The hoisted camera and the outputs of one frame: the launch's KernelArgs
// (sdf_render), or one entry of a frame sequence's table (render_frames).
// Both live in the kernel-argument segment, so every read is a scalar load.
struct ArgsView {
  KA& A;
  __device__ __forceinline__ KF inv_view() const { return A.inv_view; }
  __device__ __forceinline__ float cam(int i) const { return A.cam[i]; }
  __device__ __forceinline__ float focal() const { return A.focal; }
  __device__ __forceinline__ float aspect() const { return A.aspect; }
  __device__ __forceinline__ int32_t* steps() const { return A.steps; }
  __device__ __forceinline__ void* rgba() const { return A.rgba; }
};
struct FrameView {
  const KARG FrameCam& F;
  __device__ __forceinline__ KF inv_view() const { return F.inv_view; }
  __device__ __forceinline__ float cam(int i) const { return F.cam[i]; }
  __device__ __forceinline__ float focal() const { return F.focal; }
  __device__ __forceinline__ float aspect() const { return F.aspect; }
  __device__ __forceinline__ int32_t* steps() const { return F.steps; }
  __device__ __forceinline__ void* rgba() const { return F.rgba; }
};

// fragment main() for the pixel (x, y) of the frame V (y = 0 bottom row):
// returns its shading terms (ao, dif, x = max(N.H, 0), 1), from which
// shade.h shade_colour makes the colour, and the primary / shadow iteration
// counts in sp / ss.
// STEPS: the caller may record step counts (a kernel instantiation of its
// own: without it the per-lane iteration counts are dead after the loops,
// so no per-step copy of the uniform loop counter is made, and the exact
// shadow skip is always taken).
//
// The pixel is traced in two parts, so that a render with several lights
// (shade_pixel_lights) shares every expression with this one: trace_surface
// is what does not depend on the light -- the primary march, the normal and
// the ambient occlusion, leaving the culling state `mst` at P -- and
// light_terms is one light's (dif, x) with its shadow march from P.
struct Surface {
  V3 cam, P, N;
  float tP;   // path length at P
  float ao;
  V3 ray;     // the ray that was marched, and the distance d it went (P = cam +
  float d;    // ray d): what a reflected ray starts from (shade_pixel_reflect)
};

// trace_surface itself is two steps, so that a reflected ray (shade_pixel_reflect)
// is traced by the very code a pixel's ray is: the pixel's ray is formed
// (:191-192), then trace_ray marches from an eye along a ray and takes the
// normal and the occlusion at the point it ends on.  (The pixel's ray stays
// written out in trace_surface: as a function of its own, fast precision
// contracted its normalisations' sums of squares in another order, and every
// fast kernel's rays moved by an ulp.)
//
// trace_ray in turn is trace_march, the primary march alone (S.d, S.P, S.tP),
// and trace_shape, the normal and the occlusion at P (S.N, S.ao): a layer that
// missed the scene under a sky (shade_pixel_env) stops between the two.
// SURFACE = false ends trace_surface after the march as well.  (S.cam and
// S.ray are the caller's to fill in, and trace_ray fills the whole Surface in
// one place: with the fields written where they arise, one fast TILES kernel
// allocated two registers of its encoder the other way round.)
template <class Scene>
__device__ __forceinline__ void trace_ray(KA& A, const Scene& scene, const V3 cam, const V3 ray,
                                          int& sp, MarchState& mst, Surface& S);
template <class Scene>
__device__ __forceinline__ void trace_march(KA& A, const Scene& scene, const V3 cam, const V3 ray,
                                            int& sp, MarchState& mst, Surface& S);

template <class Scene, class View, bool SURFACE = true>
__device__ __forceinline__ void trace_surface(KA& A, const Scene& scene, const View& V, int x,
                                              int y, int& sp, MarchState& mst, Surface& S) {
  // quad = ((2x+1)/W - 1, (2y+1)/H - 1)   (voxel_geometry.geom:26-52)
#if SDF_EXACT
  // (2x+1) / W by one Markstein step from the host's RN(1/W): an integer
  // numerator in [1, 2^17) over an integer W in [1, 2^16] (A.width: the
  // sub-sample width S W of a supersampled frame, held to 2^16 as well), where
  // no step underflows or overflows (cr_math.h div_refined): the IEEE quotient
  const float qx = crm::div_refined((float)(2 * x + 1), (float)A.width, A.inv_width) - 1.0f;
  const float qy = crm::div_refined((float)(2 * y + 1), (float)A.height, A.inv_height) - 1.0f;
#else
  const float qx = (float)(2 * x + 1) * A.inv_width - 1.0f;
  const float qy = (float)(2 * y + 1) * A.inv_height - 1.0f;
#endif

  // :191-192
  V3 r0 = normalize(mk(qx * V.aspect(), qy, V.focal()));
  KF m = V.inv_view();
  V3 r1 = mk(m[0] * r0.x + m[4] * r0.y + m[8] * r0.z + m[12] * 0.0f,
             m[1] * r0.x + m[5] * r0.y + m[9] * r0.z + m[13] * 0.0f,
             m[2] * r0.x + m[6] * r0.y + m[10] * r0.z + m[14] * 0.0f);
  const V3 ray = normalize(r1);
  const V3 cam = mk(V.cam(0), V.cam(1), V.cam(2));
  if constexpr (SURFACE) {
    trace_ray(A, scene, cam, ray, sp, mst, S);
  } else {
    trace_march(A, scene, cam, ray, sp, mst, S);
    S.cam = cam;
    S.ray = ray;
  }
}

// The point the ray from `cam` along `ray` ends on (S.d: the march's
// distance, S.P = cam + ray d, S.tP the path length there).  `mst`: the culling state of a path that starts
// at `cam` (fresh), left at P.
template <class Scene>
__device__ __forceinline__ void trace_march(KA& A, const Scene& scene, const V3 cam, const V3 ray,
                                            int& sp, MarchState& mst, Surface& S) {
  const float max_dist = A.max_dist, eps = A.eps;

  // raymarch, :86-103
  float d = 0.0f;
  // Culling state along the pixel's path (FixedScene::march): the primary
  // ray, side trips to the normal and AO taps, then the shadow ray from P.
  for (; sp < A.max_steps;) {
    V3 rp = add(cam, muls(ray, d));
    float sdf = scene.march_primary(rp, d, mst);
    d += sdf;
    sp++;
    if (d > max_dist || sdf < eps) break;
  }
  const V3 P = add(cam, muls(ray, d));  // :196
  const float tP = d * kPathScale;       // path length at P
  S.P = P;
  S.tP = tP;
  S.d = d;
}

// The normal and the ambient occlusion at the point S.P a march ended on
// (`mst` its culling state there).  NORMAL = false: the normal is S.N as the
// caller set it; AO = false: no occlusion taps, S.ao = 1 (shade_points takes
// the two at different points).
template <class Scene, bool NORMAL = true, bool AO = true>
__device__ __forceinline__ void trace_shape(KA& A, const Scene& scene, MarchState& mst,
                                            Surface& S) {
  const V3 P = S.P;
  const float tP = S.tP;

  // normal, :134-155 (central) or tetrahedral
  V3 N;
  const float h = A.normal_eps;
  if constexpr (!NORMAL) {
    N = S.N;
  } else if (SDF_ABLATE_NO_NORMAL) {
    N = mk(0.0f, 1.0f, 0.0f);   // stage ablation only (tools/ablate.py): wrong pixels
  } else if (A.normal_mode == SDF_NORMAL_TETRA) {
    // taps at |h (+-1,+-1,+-1)| = |h| sqrt 3 from P: path length tt
    const float tt = tP + fabsf(h) * (1.7320509f * kPathScale);
    float f[4];
    normal_taps(scene, TetraTaps{P, h}, tP, tt, mst, f);
    N = normalize(mk(f[0] - f[1] - f[2] + f[3], -f[0] - f[1] + f[2] + f[3],
                     -f[0] + f[1] - f[2] + f[3]));
  } else {
    const float tt = tP + fabsf(h) * kPathScale;
    float f[6];
    normal_taps(scene, CentralTaps{P, h}, tP, tt, mst, f);
    N = normalize(mk(f[1] - f[0], f[3] - f[2], f[5] - f[4]));   // R - L per axis
  }

  // ambient occlusion (extension), evaluated before the shadow march so its
  // taps are side trips from P (independent of the shadow: same result)
  float ao = 1.0f;
  if constexpr (!AO) {
    S.N = N;
    S.ao = 1.0f;
    return;
  }
  const bool use_ao = (A.flags & SDF_FLAG_AO) && A.ao_taps > 0;
  if (use_ao) {
    float occ = 0.0f, sca = 1.0f;
    const int taps = A.ao_taps;
    // The taps P + N h_i lie on one line through P.  The default 5 taps run
    // as one batch, like the normal's (one culling decision per bound, tested
    // at P, for radius ao_path[4]: 1 % faster on C4 than the side path below).
    // Otherwise, visited in order, tap i is reached from P by a path of length
    // ao_path[i] = |h_0| + sum |h_k - h_(k-1)| (host fp64, rounded up), so the
    // taps are marched as one side path recording its fresh bound tests (a
    // copy of the path state: the shadow ray starts again from P).
    if (Scene::kBatchedTaps && taps == AOTaps::K) {
      float f[AOTaps::K];
      normal_taps(scene, AOTaps{P, N, A.ao_h}, tP, tP + A.ao_path[AOTaps::K - 1] * kPathScale,
                  mst, f);
#pragma unroll
      for (int i = 0; i < AOTaps::K; i++) {
        occ = occ + (A.ao_h[i] - f[i]) * sca;
        sca = sca * A.ao_falloff;
      }
    } else {
      MarchState sa = mst;
#ifdef SDF_STATS
      sa.stage = 1;
#endif
      for (int i = 0; i < taps; i++) {
        const float hh = A.ao_h[i];  // base + step * i / (taps - 1), host fp32
        float dd = scene.march(add(P, muls(N, hh)), tP + A.ao_path[i] * kPathScale, sa);
        occ = occ + (hh - dd) * sca;
        sca = sca * A.ao_falloff;
      }
    }
    ao = gclamp(1.0f - A.ao_strength * occ, 0.0f, 1.0f);
  }
  S.N = N;
  S.ao = ao;
}

// The surface the ray from `cam` along `ray` ends on: the march, then the
// normal and the occlusion there.
template <class Scene>
__device__ __forceinline__ void trace_ray(KA& A, const Scene& scene, const V3 cam, const V3 ray,
                                          int& sp, MarchState& mst, Surface& S) {
  Surface T;
  trace_march(A, scene, cam, ray, sp, mst, T);
  trace_shape(A, scene, mst, T);
  S.cam = cam;
  S.P = T.P;
  S.N = T.N;
  S.tP = T.tP;
  S.ao = T.ao;
  S.ray = ray;
  S.d = T.d;
}

// A path's ray (shade_pixel_reflect, shade_pixel_env, shade_ray: O_j, D_j of a
// reflected layer) may have components that are not finite: a normal that is
// normalize(0) -- far from the origin, where the taps P +- normal_eps all
// round to P -- is NaN, and so are the ray mirrored at it and its origin.  The
// path "goes on as the arithmetic says" (sdf_abi.h "Reflections"), the
// arithmetic of the scene spec with its selects, which the scene evaluators
// do not keep on a NaN point (see sel_query below: sdf_trace's rays of this
// kind).  So a lane with such a ray takes its primary march through sel_scene,
// operation for operation the CPU oracle's raymarch: d_j, P_j and the primary
// step count are the oracle's.  Its culling state stays the fresh one.  A cold
// path behind a real branch, entered by a wave only when one of its lanes has
// such a ray; primitive scenes only, as there.
__device__ __forceinline__ float sel_scene(KA& A, V3 p);
template <class Scene>
__device__ __forceinline__ void trace_march_path(KA& A, const Scene& scene, const V3 cam,
                                                 const V3 ray, int& sp, MarchState& mst,
                                                 Surface& S) {
  const bool odd = !(fabsf(ray.x) < INFINITY && fabsf(ray.y) < INFINITY &&
                     fabsf(ray.z) < INFINITY && fabsf(cam.x) < INFINITY &&
                     fabsf(cam.y) < INFINITY && fabsf(cam.z) < INFINITY);
  if (A.scene_kind == SDF_SCENE_PRIMITIVES && __builtin_amdgcn_ballot_w64(odd) != 0) {
    asm volatile("" ::: "memory");   // a real branch: never if-converted into the march
    if (odd) {
      float d = 0.0f;
#pragma unroll 1
      for (; sp < A.max_steps;) {
        const float s = sel_scene(A, add(cam, muls(ray, d)));
        d += s;
        sp++;
        if (d > A.max_dist || s < A.eps) break;
      }
      S.P = add(cam, muls(ray, d));
      S.tP = d * kPathScale;
      S.d = d;
      return;
    }
  }
  trace_march(A, scene, cam, ray, sp, mst, S);
}
// trace_ray for such a ray
template <class Scene>
__device__ __forceinline__ void trace_ray_path(KA& A, const Scene& scene, const V3 cam,
                                               const V3 ray, int& sp, MarchState& mst,
                                               Surface& S) {
  Surface T;
  trace_march_path(A, scene, cam, ray, sp, mst, T);
  trace_shape(A, scene, mst, T);
  S.cam = cam;
  S.P = T.P;
  S.N = T.N;
  S.tP = T.tP;
  S.ao = T.ao;
  S.ray = ray;
  S.d = T.d;
}

// The terms of the light at Lp for the surface S: dif = clamp(N.L, 0, 1) *
// shadow and spec_x = max(N.H, 0); `mst` is the culling state at P (advanced
// along the shadow ray), `ss` counts the shadow march's iterations from 0.
//
// `hook` (surface_colour's, handed on) sees what a render keeps to itself:
// NoLightHook, the default, is empty, and every kernel without one of its own
// compiles to the code it had before there were hooks (PointsHook below: what a
// hook has).
struct NoLightHook {
  static constexpr bool kOn = false;   // every use of a hook stands behind if constexpr (kOn)
};
template <bool STEPS, class Scene, class View, class Hook = NoLightHook>
__device__ __forceinline__ void light_terms(KA& A, const Scene& scene, const View& V,
                                            const Surface& S, const V3 Lp, MarchState& mst,
                                            int& ss, float& dif_out, float& spec_x_out,
                                            const Hook* hook = nullptr) {
  const V3 cam = S.cam, P = S.P, N = S.N;
  const float tP = S.tP;
  const float max_dist = A.max_dist, eps = A.eps;
  // Blinn-Phong, :200-204
#if SDF_EXACT
  const V3 view = normalize(sub(cam, P));
  const V3 incident = normalize(sub(Lp, P));
  const V3 halfway = normalize(add(incident, view));
#else
  const V3 incident = normalize(sub(Lp, P));
  // incident + normalize(cam - P) with the view's scaling fused into the sum:
  // what contraction makes of it where both stand in one block, as in every
  // single-light kernel.  Written out, because the loop over several lights
  // hoists the light-independent `view` as rounded products and would add it
  // unfused: x one ulp apart on ~10 % of the pixels.  (The view is recomputed
  // per light instead of kept live: a subtraction, a v_rsq and three FMAs.)
  const V3 cp = sub(cam, P);
  const float rv = frsqrt(dot(cp, cp));
  const V3 halfway = normalize(mk(__builtin_fmaf(cp.x, rv, incident.x),
                                  __builtin_fmaf(cp.y, rv, incident.y),
                                  __builtin_fmaf(cp.z, rv, incident.z)));
#endif
  const float spec_x = gmax(dot(N, halfway), 0.0f);   // spec = pow(spec_x, shininess)

  // soft shadow, :105-132, :205
  float sh = 1.0f;
  // When clamp(dot(N, L), 0, 1) is 0 (or NaN) the diffuse term is 0 * sh (or
  // NaN) for every sh in [0, 1]: the march cannot change the pixel and is
  // skipped -- unless the caller asked for the reference step counts.
  const float ndl = dot(N, incident);
  if ((A.flags & SDF_FLAG_SHADOW) && ((STEPS && V.steps() != nullptr) || ndl > 0.0f)) {
    const float off = A.shadow_offset, k = A.shadow_k;
    const V3 o = mk(P.x + N.x * off * eps, P.y + N.y * off * eps, P.z + N.z * off * eps);
    float t = 0.0f, hprev = INFINITY, s = 1.0f;
#if !SDF_EXACT
    float hhprev = INFINITY;
#endif
    const float to = tP + fabsf(off * eps) * kPathScale;   // path length at the origin
#ifdef SDF_STATS
    mst.stage = 2;
#endif
    // the march's lit tail (FixedScene::shadow_limit): ends it as soon as no
    // later step can change the shadow -- unless step counts are recorded
    float tlim = max_dist;
    bool lit = false;
    if constexpr (Scene::kPlaneHead) {
      if (!(STEPS && V.steps() != nullptr)) tlim = scene.shadow_limit(o, incident, k, max_dist, lit);
    }
#if SDF_EXACT
    // k (1 - 2^-20) for the step's lower bound of k dest (a negative k: no
    // bound, every step takes the exact path)
    const float k_lo = k >= 0.0f ? k * 0x1.ffffep-1f : -INFINITY;
#endif
    if (!lit)
    for (; ss < A.max_steps;) {
      V3 rp = add(o, muls(incident, t));
      float hn = scene.march(rp, to + t * kPathScale, mst);
#if SDF_EXACT
      const float hh = hn * hn;
      // The step's term k dest / den is formed exactly (IEEE division
      // of hn^2 by 2 h_prev, cr_sqrt, ...) only when some lane of the wave may
      // lower s with it.  Step 0 never does (t = 0: den = +0, the term is
      // +INF or NaN).  Later steps first bound the term from below without the
      // division: r = v_rcp(2 h_prev) for 2 h_prev in [2^-100, 2^100) (1 ulp,
      // normal), ia = RN(hn^2 r) within 2^-22 relative (2^-150 absolute if
      // subnormal) of the oracle's inter = RN(hn^2 / (2 h_prev)), so ihi =
      // ia (1 + 2^-19) + 2^-125 >= inter >= ilo = ia (1 - 2^-19) - 2^-125;
      // squaring and RN are monotone, so RN(hn^2 - RN(ihi^2)) <= the oracle's
      // RN(hn^2 - RN(inter^2)), and v_sqrt (1 ulp) times k (1 - 2^-20) is
      // below its num = RN(k RN(sqrt(.))) by more than the roundings;
      // RN(t - ilo) >= RN(t - inter), so >= den.  When RN(numlo - s denhi)
      // >= 2^-100 (every bound above in the normal range) on every lane, num
      // > s den, so RN(num / den) >= s (or den = +0: +INF / NaN) and min
      // keeps s: the exact term is skipped, bit for bit the same.  NaN
      // anywhere fails the test.  tools/block_counts.py: the IEEE division
      // was ~95 VALU per wave on C4 exact.
      bool skip = ss == 0;
      if (!skip) {
        const float d2 = 2.0f * hprev;
        const float ia = hh * __builtin_amdgcn_rcpf(d2);
        const float ihi = __builtin_fmaf(ia, 0x1.00002p0f, 0x1p-125f);
        const float ilo = __builtin_fmaf(ia, 0x1.ffffcp-1f, -0x1p-125f);
        const float numlo = __builtin_amdgcn_sqrtf(hh - ihi * ihi) * k_lo;
        const float denhi = t - ilo;
        const bool ok = (__float_as_uint(d2) - 0x0D800000u) < (0x71800000u - 0x0D800000u) &&
                        __builtin_fmaf(-s, denhi, numlo) >= 0x1p-100f;
        skip = __builtin_amdgcn_ballot_w64(!ok) == 0;
      }
      if (!skip) {
        float inter = (ss == 0) ? 0.0f : fdiv(hh, 2.0f * hprev);
        float dest = fsqrt(hh - inter * inter);
        // t - inter may be NaN (then both keep +0) but never -0 against +0
        // ordered differently: max(+0, y) is +0 for y <= 0 either way
        const float num = k * dest, den = hw_max(0.0f, t - inter);
        // gmin(s, RN(num / den)) is s wherever RN(num - s den) > 0: then num /
        // den > s exactly (den > 0), so its rounding is >= s; num > 0 = den
        // gives +INF (s is never NaN or above 1).  So the IEEE division runs
        // only when some lane of the wave may lower s -- bit for bit the same
        // (C4 exact 2.6-3.3 % faster).
        if (__builtin_amdgcn_ballot_w64(!(__builtin_fmaf(-s, den, num) > 0.0f)) != 0)
          // s in [-inf, 1] is never NaN or -0; num / den >= +0 or NaN (num >=
          // +0: k > 0, dest a square root; den >= +0), and NaN keeps s both ways
          s = hw_min(s, fdiv(num, den));
      }
#else
      // The same term with inter = h^2 / (2 hp) eliminated:
      //   k dest / (t - inter) = k |h| sqrt(4 hp^2 - h^2) / (2 |hp| t - sgn(hp) h^2)
      // (one sqrt and one rcp per step instead of two rcp and a sqrt).  A
      // denominator <= 0 (t <= inter) selects rcp(0) = +INF as max(0, .) does;
      // 4 hp^2 < h^2 gives NaN as hn^2 - inter^2 < 0 does (ignored by the min);
      // step 0 (hp = INF, t = 0) gives k |h| * INF, as k |h| / 0 does.
      const float hh = hn * hn;
      const float num = k * fabsf(hn) * __builtin_amdgcn_sqrtf(__builtin_fmaf(4.0f, hhprev, -hh));
      const float den = __builtin_fmaf(2.0f * fabsf(hprev), t, -__builtin_copysignf(hh, hprev));
      s = acc_min(s, num * __builtin_amdgcn_rcpf(den > 0.0f ? den : 0.0f));
      hhprev = hh;
#endif
      hprev = hn;
      t += hn;
      ss++;
      if (t > tlim || s < eps) break;
    }
    sh = gclamp(s, 0.0f, 1.0f);
  }
  if constexpr (Hook::kOn) hook->shadow(sh);
  dif_out = gclamp(ndl, 0.0f, 1.0f) * sh;
  spec_x_out = spec_x;
}

template <bool STEPS, class Scene, class View>
__device__ __forceinline__ float4 shade_pixel(KA& A, const Scene& scene, const View& V, int x,
                                              int y, int& sp, int& ss) {
  MarchState mst;
  Surface S;
  trace_surface(A, scene, V, x, y, sp, mst, S);
  float dif, spec_x;
  light_terms<STEPS>(A, scene, V, S, mk(A.light_pos[0], A.light_pos[1], A.light_pos[2]), mst, ss,
                     dif, spec_x);
  // ambient (+ AO extension) and the colour sum, :206-210: shade.h
  return make_float4(S.ao, dif, spec_x, 1.0f);
}

// The pixel's colour under the launch's L.n lights (sdf_abi.h "Lights"): the
// surface is traced once, then every light adds its diffuse and specular to
// the three channels in index order.  Each light's shadow march starts from
// a copy of the culling state the single-light kernel has at P, and its
// terms come from the very light_terms above, so (dif_i, x_i) are the bits
// sdf_render gives with that light alone.  The count, the colour flag and
// the lights are uniforms of the kernel-argument segment: one kernel serves
// every L, and the loop reads scalars.  `ss` sums the lights' shadow counts.
// (trace_surface plus surface_colour<STEPS, false> below was tried: the same
// bits and registers, but every render_lights kernel's schedule moved and C4
// at 1080p ran 1.1-1.5 % slower in both precisions, so the loop stays here.)
template <bool STEPS, class Scene, class View>
__device__ __forceinline__ float4 shade_pixel_lights(KA& A, const KARG LightsArgs& L,
                                                     const Scene& scene, const View& V, int x,
                                                     int y, int& sp, int& ss) {
  MarchState mst;
  Surface S;
  trace_surface(A, scene, V, x, y, sp, mst, S);
  float acc[3];
#pragma unroll
  for (int c = 0; c < 3; c++) acc[c] = shade_ambient(L.la * A.mat_amb[c], S.ao);
  const bool tint = (L.flags & SDF_LIGHTS_COLOR) != 0;
  const int n = L.n;
#pragma unroll 1
  for (int i = 0; i < n; i++) {
    MarchState ms = mst;
    int ssi = 0;
    float dif, spec_x;
    light_terms<STEPS>(A, scene, V, S, mk(L.pos[i][0], L.pos[i][1], L.pos[i][2]), ms, ssi, dif,
                       spec_x);
    ss += ssi;
    const float spec = spec_pow<SDF_EXACT>(spec_x, A.shininess);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float d = tint ? shade_tint(dif, L.color[i][c]) : dif;
      const float s = tint ? shade_tint(spec, L.color[i][c]) : spec;
      acc[c] = shade_light<SDF_EXACT>(acc[c], A.mat_dif[c], A.mat_ref[c], d, s);
    }
  }
  return make_float4(acc[0], acc[1], acc[2], 1.0f);
}

// shade_pixel_lights with a material per primitive (sdf_abi.h "Materials"):
// between the surface and the lights the scene's material fold runs once at
// P and leaves the pixel's blended amb, dif and ref.  The ambient part goes
// into the channel sums at once, so only dif and ref (6 values) live across
// the shadow marches.  trace_surface and light_terms are the shared ones:
// P, N, ao, (dif_i, x_i) and the step counts are sdf_render_lights's bits.
// (trace_surface plus surface_colour<STEPS, true> below was tried: the same
// bits and registers, the fast kernels 1 % faster, but the exact ones 1.1-1.6 %
// slower on C4 at 1080p, so the fold and the loop stay here.)
template <bool STEPS, class Scene, class View>
__device__ __forceinline__ float4 shade_pixel_materials(KA& A, const KARG LightsArgs& L,
                                                        const KARG MaterialArgs& M,
                                                        const Scene& scene, const View& V, int x,
                                                        int y, int& sp, int& ss) {
  MarchState mst;
  Surface S;
  trace_surface(A, scene, V, x, y, sp, mst, S);
  float acc[3], md[3], mr[3];
  {
    float m[9];
#pragma unroll
    for (int c = 0; c < 9; c++) m[c] = M.m[0][c];
    scene.material_fold(S.P, M, m);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      acc[c] = shade_ambient(shade_tint(L.la, m[c]), S.ao);
      md[c] = m[3 + c];
      mr[c] = m[6 + c];
    }
  }
  const bool tint = (L.flags & SDF_LIGHTS_COLOR) != 0;
  const int n = L.n;
#pragma unroll 1
  for (int i = 0; i < n; i++) {
    MarchState ms = mst;
    int ssi = 0;
    float dif, spec_x;
    light_terms<STEPS>(A, scene, V, S, mk(L.pos[i][0], L.pos[i][1], L.pos[i][2]), ms, ssi, dif,
                       spec_x);
    ss += ssi;
    const float spec = spec_pow<SDF_EXACT>(spec_x, A.shininess);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float d = tint ? shade_tint(dif, L.color[i][c]) : dif;
      const float s = tint ? shade_tint(spec, L.color[i][c]) : spec;
      acc[c] = shade_light<SDF_EXACT>(acc[c], md[c], mr[c], d, s);
    }
  }
  return make_float4(acc[0], acc[1], acc[2], 1.0f);
}

// A surface's colour under the launch's L.n lights (sdf_abi.h "Lights",
// "Materials"): the ambient part, then every light adds its diffuse and
// specular to the three channels in index order.  Each light's shadow march
// starts from a copy of the culling state the single-light kernel has at P,
// and its terms come from the very light_terms above, so (dif_i, x_i) are the
// bits sdf_render gives with that light alone.  The count, the colour flag
// and the lights are uniforms of the kernel-argument segment: one kernel
// serves every L, and the loop reads scalars.  `ss` sums the lights' shadow
// counts.
//
// FOLD: a material per primitive -- the scene's material fold runs once at P
// and leaves the surface's blended amb, dif and ref; else the frame's one
// material (KernelArgs).  The ambient part goes into the channel sums at
// once, so only dif and ref (6 values) live across the shadow marches.  `mr`
// (the ref used) is handed back for a reflecting path's weights.
//
// It is shade_pixel_materials's (FOLD) and shade_pixel_lights's statements
// after trace_surface, for the reflect and env kernels' layers.
//
// `hook` (NoLightHook: none) may skip the fold and the loop, take spec_i = +0
// for a surface without an eye, and see the blended components and each
// light's shadow factor and count: shade_points's outputs.
template <bool STEPS, bool FOLD, class Scene, class View, class Hook = NoLightHook>
__device__ __forceinline__ void surface_colour(KA& A, const KARG LightsArgs& L,
                                               const KARG MaterialArgs& M, const Scene& scene,
                                               const View& V, const Surface& S,
                                               const MarchState& mst, int& ss, float (&acc)[3],
                                               float (&mr)[3], const Hook* hook = nullptr) {
  float md[3];
  if constexpr (FOLD) {
    float m[9];
#pragma unroll
    for (int c = 0; c < 9; c++) m[c] = M.m[0][c];
    if constexpr (Hook::kOn) {
      if (hook->fold()) scene.material_fold(S.P, M, m);
      hook->material(m);
    } else {
      scene.material_fold(S.P, M, m);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      acc[c] = shade_ambient(shade_tint(L.la, m[c]), S.ao);
      md[c] = m[3 + c];
      mr[c] = m[6 + c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      acc[c] = shade_ambient(shade_tint(L.la, A.mat_amb[c]), S.ao);
      md[c] = A.mat_dif[c];
      mr[c] = A.mat_ref[c];
    }
  }
  const bool tint = (L.flags & SDF_LIGHTS_COLOR) != 0;
  const int n = L.n;
#pragma unroll 1
  for (int i = 0; i < n; i++) {
    if constexpr (Hook::kOn) {
      if (!hook->lights()) break;   // a uniform: no light loop at all
    }
    MarchState ms = mst;
    int ssi = 0;
    float dif, spec_x;
    if constexpr (Hook::kOn) {
      light_terms<STEPS>(A, scene, V, S, mk(L.pos[i][0], L.pos[i][1], L.pos[i][2]), ms, ssi, dif,
                         spec_x, hook);
      hook->light(i, ssi);
    } else {
      light_terms<STEPS>(A, scene, V, S, mk(L.pos[i][0], L.pos[i][1], L.pos[i][2]), ms, ssi, dif,
                         spec_x);
    }
    ss += ssi;
    float spec;
    if constexpr (Hook::kOn) {
      spec = 0.0f;
      if (hook->eye()) spec = spec_pow<SDF_EXACT>(spec_x, A.shininess);
    } else {
      spec = spec_pow<SDF_EXACT>(spec_x, A.shininess);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float d = tint ? shade_tint(dif, L.color[i][c]) : dif;
      const float s = tint ? shade_tint(spec, L.color[i][c]) : spec;
      acc[c] = shade_light<SDF_EXACT>(acc[c], md[c], mr[c], d, s);
    }
  }
}

// The pixel's path of mirror bounces (sdf_abi.h "Reflections"): layer j is the
// materials pipeline above for the fragment whose eye is O_j and whose ray is
// D_j -- trace_ray, then surface_colour (FOLD: the material fold at P_j; a
// Mandelbulb has the one material of KernelArgs) with the view from O_j, the
// colour sum C_j -- and the next ray leaves P_j + N_j offset eps, the shadow
// march's origin, along D_j mirrored at N_j.

// What a path carries from layer to layer: the next ray, the weights W_j,
// the output and the step counts, and whether the lane's path goes on.
//   composite (layer < 0): acc = C_0, then acc += W_j C_j in the precision's
//   form; sp / ss sum the layers' counts.  One layer: acc = C_layer (or
//   W_layer), sp / ss that layer's; a path that ended before it leaves zeros.
struct ReflectPath {
  V3 O = {0.0f, 0.0f, 0.0f}, D = {0.0f, 0.0f, 0.0f};
  float W[3] = {1.0f, 1.0f, 1.0f};
  float acc[3] = {0.0f, 0.0f, 0.0f};
  int sp = 0, ss = 0;
  bool live = true;
  // layer j is traced: S its surface (S.d its march's distance), C its
  // colour, mr its blended ref, spj / ssj its counts.  ENV (shade_pixel_env)
  // with `fog` (SDF_ENV_FOG, a uniform): what lies behind the layer is
  // attenuated by its fog factor f as well, a second rounded product.
  template <bool ENV = false>
  __device__ __forceinline__ void layer_done(KA& A, const KARG ReflectArgs& R, int j,
                                             const Surface& S, const float (&C)[3],
                                             const float (&mr)[3], int spj, int ssj,
                                             float f = 1.0f, bool fog = false) {
    const int want = R.layer;
    if (want < 0) {
#pragma unroll
      for (int c = 0; c < 3; c++)
        acc[c] = j == 0 ? C[c] : reflect_add<SDF_EXACT>(acc[c], W[c], C[c]);
      sp += spj;
      ss += ssj;
    } else if (j == want) {
#pragma unroll
      for (int c = 0; c < 3; c++) acc[c] = R.weight ? W[c] : C[c];
      sp = spj;
      ss = ssj;
    }
    // W_(j+1), and whether the path goes on: not past the last layer wanted,
    // not off a miss, not off a surface that reflects nothing (a NaN weight
    // is not 0: the path goes on)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      W[c] = shade_tint(W[c], shade_tint(R.strength, mr[c]));
      if constexpr (ENV) {
        if (fog) W[c] = shade_tint(W[c], f);
      }
    }
    const int last = want >= 0 ? want : R.bounces;
    live = j < last && !(S.d > A.max_dist) && !(W[0] == 0.0f && W[1] == 0.0f && W[2] == 0.0f);
    // the next ray: D mirrored at N (no branch on the sign of N.D), from the
    // shadow march's origin (light_terms `o`)
    const V3 N = S.N, P = S.P;
    const float s2 = 2.0f * dot(N, D);
    D = normalize(mk(D.x - s2 * N.x, D.y - s2 * N.y, D.z - s2 * N.z));
    const float off = A.shadow_offset, eps = A.eps;
    O = mk(P.x + N.x * off * eps, P.y + N.y * off * eps, P.z + N.z * off * eps);
  }
};

// Layer 0 stands in front of the loop over the reflected layers and is
// trace_surface, its eye the uniform camera, then surface_colour, so that
// fast precision contracts it the way the materials kernels do (layer 0 IS
// their pixel: tests/test_gpu_reflect.py holds the bits); the loop's layers
// take their eye per lane.  (One loop body for every layer, layer 0's eye the
// camera moved into VGPRs, measured 2-4 % faster, but in fast precision the
// generic kernel's
// layer 0 then came out a few ulps off sdf_render_materials's: DESIGN.md,
// Reflections.)  Each layer starts a fresh culling state: the path length a
// MarchState measures restarts at O_j, which is conservative like the first
// ray's.  The loop's exit is per lane (a pixel whose path has ended idles), so
// the wave leaves it when no lane is live.  bounces, layer, the weight flag
// and the strength are uniforms: one kernel serves them all.
template <bool STEPS, bool FOLD, class Scene, class View>
__device__ __forceinline__ float4 shade_pixel_reflect(KA& A, const KARG LightsArgs& L,
                                                      const KARG MaterialArgs& M,
                                                      const KARG ReflectArgs& R,
                                                      const Scene& scene, const View& V, int x,
                                                      int y, int& sp, int& ss) {
  ReflectPath path;
  {
    MarchState mst;
    Surface S;
    int spj = 0, ssj = 0;
    trace_surface(A, scene, V, x, y, spj, mst, S);
    float C[3], mr[3];
    surface_colour<STEPS, FOLD>(A, L, M, scene, V, S, mst, ssj, C, mr);
    path.D = S.ray;
    path.layer_done(A, R, 0, S, C, mr, spj, ssj);
  }
#pragma unroll 1
  for (int j = 1; path.live; j++) {
    MarchState mst;
    Surface S;
    int spj = 0, ssj = 0;
    trace_ray_path(A, scene, path.O, path.D, spj, mst, S);
    float C[3], mr[3];
    surface_colour<STEPS, FOLD>(A, L, M, scene, V, S, mst, ssj, C, mr);
    path.layer_done(A, R, j, S, C, mr, spj, ssj);
  }
  sp = path.sp;
  ss = path.ss;
  return make_float4(path.acc[0], path.acc[1], path.acc[2], 1.0f);
}

// The path above with an environment (sdf_abi.h "Environment").  env_layer is
// what follows a layer's march: the miss test d_j > max_dist, the comparison
// that ends the path, stands between trace_march and the surface work.  Under
// SDF_ENV_SKY a missed lane takes the sky along its ray (shade.h env_sky) and
// skips the normal, the occlusion taps, the material fold and every light
// behind a real branch, so a wave whose lanes all miss runs none of them;
// lanes of a mixed wave idle as ended paths do.  With SDF_ENV_FOG every other
// layer's colour is moved towards the fog colour by its factor f (env_fog),
// which also enters the next weight.  A sky layer has no surface: its path
// ends there (the miss), its ref is 0 and its shadow count 0.
template <bool STEPS, bool FOLD, class Scene, class View>
__device__ __forceinline__ void env_layer(KA& A, const KARG LightsArgs& L,
                                          const KARG MaterialArgs& M,
                                          const KARG ReflectArgs& R, const KARG EnvArgs& E,
                                          const Scene& scene, const View& V, int j, Surface& S,
                                          MarchState& mst, int spj, ReflectPath& path) {
  const bool fog = (E.flags & SDF_ENV_FOG) != 0;
  const bool sky = (E.flags & SDF_ENV_SKY) != 0 && S.d > A.max_dist;
  float C[3], mr[3] = {0.0f, 0.0f, 0.0f};
  float f = 1.0f;
  int ssj = 0;
  if (sky) {
    const float D[3] = {S.ray.x, S.ray.y, S.ray.z};
    const float hz[3] = {E.horizon[0], E.horizon[1], E.horizon[2]};
    const float ze[3] = {E.zenith[0], E.zenith[1], E.zenith[2]};
    const float gr[3] = {E.ground[0], E.ground[1], E.ground[2]};
    const float sd[3] = {E.sun_dir[0], E.sun_dir[1], E.sun_dir[2]};
    const float sc[3] = {E.sun_color[0], E.sun_color[1], E.sun_color[2]};
    env_sky<SDF_EXACT>(D, hz, ze, gr, (E.flags & SDF_ENV_SUN) != 0, sd, sc, E.sun_exponent, C);
    S.N = mk(0.0f, 0.0f, 0.0f);
    S.ao = 1.0f;
  } else {
    trace_shape(A, scene, mst, S);
    surface_colour<STEPS, FOLD>(A, L, M, scene, V, S, mst, ssj, C, mr);
    if (fog) {
      f = env_fog<SDF_EXACT>(S.d, E.fog_end, E.fog_den, E.fog_inv);
#pragma unroll
      for (int c = 0; c < 3; c++) C[c] = material_mix<SDF_EXACT>(E.fog_color[c], C[c], f);
    }
  }
  path.template layer_done<true>(A, R, j, S, C, mr, spj, ssj, f, fog);
}

template <bool STEPS, bool FOLD, class Scene, class View>
__device__ __forceinline__ float4 shade_pixel_env(KA& A, const KARG LightsArgs& L,
                                                  const KARG MaterialArgs& M,
                                                  const KARG ReflectArgs& R,
                                                  const KARG EnvArgs& E, const Scene& scene,
                                                  const View& V, int x, int y, int& sp, int& ss) {
  ReflectPath path;
  {
    MarchState mst;
    Surface S;
    int spj = 0;
    trace_surface<Scene, View, false>(A, scene, V, x, y, spj, mst, S);
    path.D = S.ray;
    env_layer<STEPS, FOLD>(A, L, M, R, E, scene, V, 0, S, mst, spj, path);
  }
#pragma unroll 1
  for (int j = 1; path.live; j++) {
    MarchState mst;
    Surface S;
    int spj = 0;
    trace_march_path(A, scene, path.O, path.D, spj, mst, S);
    S.cam = path.O;
    S.ray = path.D;
    env_layer<STEPS, FOLD>(A, L, M, R, E, scene, V, j, S, mst, spj, path);
  }
  sp = path.sp;
  ss = path.ss;
  return make_float4(path.acc[0], path.acc[1], path.acc[2], 1.0f);
}

// The frame's shading constants (shade.h), as every pixel's colour uses them
__device__ __forceinline__ ShadeK frame_shade(KA& A) {
  ShadeK K;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    K.lam[c] = A.light_amb * A.mat_amb[c];
    K.dif[c] = A.mat_dif[c];
    K.ref[c] = A.mat_ref[c];
  }
  K.shin = A.shininess;
  return K;
}
// What a pixel stores: its terms for SHADE32F, else its colour
__device__ __forceinline__ float4 pixel_value(KA& A, int format, float4 t) {
  if (format == SDF_FORMAT_SHADE32F) return t;
  return shade_colour<SDF_EXACT>(frame_shade(A), t.x, t.y, t.z);
}

// ---- supersampling resolve (sdf_abi.h sdf_params.samples) ------------------
// The wave's 8x8 tile holds whole S x S groups of sub-samples (S = 2 or 4, a
// uniform): lane bits 0, 1 carry a sub-sample's x inside the tile and bits 3,
// 4 its y.  One channel's group sum in the contract's order -- a balanced
// pairwise tree, first along x, then along y, left / lower operand first:
//   S = 2   h_j = c[0][j] + c[1][j];                      (h_0 + h_1)
//   S = 4   a_j = (c[0][j] + c[1][j]) + (c[2][j] + c[3][j]);
//           (a_0 + a_1) + (a_2 + a_3)
// by adding the xor-partner's value (wave_bits.h: DPP quad_perm for 1 and 2,
// ds_swizzle for 8 and 16).  The group's (0, 0) lane is the left / lower
// operand of every addition it makes, so it ends with the tree's value; the
// other lanes' sums are not used.  Plain fp32 additions, never fused.
// (The exchanges for 8 and 16 as VALU moves instead -- DPP row_ror:8 and
// v_permlane16_swap -- measured no faster, DESIGN.md: the LDS round trips at
// the wave's end are not what the epilogue costs.)
__device__ __forceinline__ float ssaa_sum(float v, bool four) {
#pragma clang fp contract(off)
  v = v + __uint_as_float(xor_partner<1>(__float_as_uint(v)));
  if (four) v = v + __uint_as_float(xor_partner<2>(__float_as_uint(v)));
  v = v + __uint_as_float(xor_partner<8>(__float_as_uint(v)));
  if (four) v = v + __uint_as_float(xor_partner<16>(__float_as_uint(v)));
  return v;
}

// TILES: the output is the TILES wire format (a separate instantiation, so
// the encoder's registers never weigh on the plain-format kernels)
// SSAA: the lanes are the sub-samples of a supersampled frame and the output
// is their resolved pixels (render_ssaa, an instantiation of its own as well)
// LIGHTS: the pixel's colour is the sum over the launch's lights
// (shade_pixel_lights; render_lights, instantiations of their own)
// MATERIALS (with LIGHTS): a material per primitive, blended at P
// (shade_pixel_materials; render_materials, instantiations of their own)
// REFLECT (with LIGHTS; MATERIALS: the scene has a primitive list to fold
// over): the pixel's path of mirror bounces (shade_pixel_reflect;
// render_reflect, instantiations of their own)
// ENV (with REFLECT): the path with a sky for missed layers and distance fog
// (shade_pixel_env; render_env, instantiations of their own)
template <class Scene, bool TILES, bool STEPS, bool SSAA = false, bool LIGHTS = false,
          bool MATERIALS = false, bool REFLECT = false, bool ENV = false>
__device__ __forceinline__ void render_body() {
  static_assert(!(TILES && SSAA), "a TILES stream carries shading terms, not colours");
  static_assert(!(TILES && LIGHTS), "a TILES stream carries one light's terms");
  static_assert(LIGHTS || !MATERIALS, "the materials kernels are lights kernels");
  static_assert(LIGHTS || !REFLECT, "the reflect kernels are lights kernels");
  static_assert(REFLECT || !ENV, "the env kernels are reflect kernels");
  const KARG char* const seg = (const KARG char*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = *(KA*)seg;
  const KARG RowOrder& O = *(const KARG RowOrder*)(seg + __builtin_offsetof(RenderArgs, o));
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int x = blockIdx.x * (8 * kWgWaves) + wave * 8 + (lane & 7);
  // the packed 8-row block of this row of workgroups: a schedule's order
  // (kernel_args.h RowOrder: the costliest blocks of earlier frames first),
  // else bottom-up (static middle-out and top-down orders measured slower on
  // C3/C4, profiles/r04_ab_row_order.json)
  const int by = O.n > 0 ? (int)O.order[blockIdx.y] : (int)blockIdx.y;
  const unsigned long long t_start = O.cost ? __builtin_amdgcn_s_memtime() : 0ull;
  const int pr = by * 8 + (lane >> 3);
  const bool valid = x < A.width && pr < A.rows;
  if constexpr (!TILES) {
    // SSAA: a group of S x S sub-samples leaves whole or not at all.  The
    // tile starts at multiples of 8 in x and in packed rows and 8 is a
    // multiple of S, so a group never straddles a wave; A.width = S W and
    // A.rows = S rows are multiples of S, and so is every run of packed rows
    // (block_rows and the frame's last row are S times the request's), so a
    // group lies wholly inside or wholly outside the frame and inside one
    // tiling block: its lanes share `valid` and consecutive frame rows, and
    // the resolve below exchanges values among lanes that are all present.
    if (!valid) return;
  } else {
    // every lane of a wave with a pixel in the frame stays: the tile encoder
    // is a wave-wide operation (store_tiles)
    if (blockIdx.x * kWgWaves + wave >= ((A.width + 7) >> 3)) return;
  }
  // packed row -> frame row: period blk, row `within` of its run of blocks.
  // A run of a multiple of 8 rows (every tiling of 8-row blocks) holds the
  // wave's 8 packed rows whole: its period and offset are wave-uniform,
  // scalar arithmetic (the per-lane integer division was ~20 VALU per wave,
  // tools/block_counts.py)
  int y;
  const int r0 = by * 8;
  if ((A.chunk_rows & 7) == 0) {
    const int blk0 = r0 / A.chunk_rows;
    y = (A.first_block + blk0 * A.block_stride) * A.block_rows + (r0 - blk0 * A.chunk_rows) +
        (lane >> 3);
  } else {
    const int blk = pr / A.chunk_rows;
    const int within = pr - blk * A.chunk_rows;
    y = (A.first_block + blk * A.block_stride) * A.block_rows + within;
  }
  if (A.run_gap_rows) {
    // spaced runs (sdf_tiling.run_step): block_rows % 8 == 0, so the wave's
    // 8 packed rows lie in one block, found with scalar arithmetic
    const int w0 = r0 - (r0 / A.chunk_rows) * A.chunk_rows;
    y += (w0 / A.block_rows) * A.run_gap_rows;
  }
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
  int sp = 0, ss = 0;
  if (valid) {
    const Scene scene(A);
    if constexpr (LIGHTS) {
      const KARG LightsArgs& L =
          *(const KARG LightsArgs*)(seg + __builtin_offsetof(RenderArgs, l));
      if constexpr (REFLECT) {
        const KARG MaterialArgs& M =
            *(const KARG MaterialArgs*)(seg + __builtin_offsetof(RenderArgs, m));
        const KARG ReflectArgs& R =
            *(const KARG ReflectArgs*)(seg + __builtin_offsetof(RenderArgs, r));
        if constexpr (ENV) {
          const KARG EnvArgs& E =
              *(const KARG EnvArgs*)(seg + __builtin_offsetof(RenderArgs, e));
          c = shade_pixel_env<STEPS, MATERIALS>(A, L, M, R, E, scene, ArgsView{A}, x, y, sp, ss);
        } else {
          c = shade_pixel_reflect<STEPS, MATERIALS>(A, L, M, R, scene, ArgsView{A}, x, y, sp,
                                                    ss);
        }
      } else if constexpr (MATERIALS) {
        const KARG MaterialArgs& M =
            *(const KARG MaterialArgs*)(seg + __builtin_offsetof(RenderArgs, m));
        c = shade_pixel_materials<STEPS>(A, L, M, scene, ArgsView{A}, x, y, sp, ss);
      } else {
        c = shade_pixel_lights<STEPS>(A, L, scene, ArgsView{A}, x, y, sp, ss);   // the colour
      }
    } else {
      c = shade_pixel<STEPS>(A, scene, ArgsView{A}, x, y, sp, ss);
    }
  }
  const size_t o = (size_t)(A.frame_rows ? y : pr) * A.width + x;
  if (O.cost) {
    // this wave's cycles to its block (one lane: a vector atomic)
    const unsigned long long dt = __builtin_amdgcn_s_memtime() - t_start;
    if (lane == (int)__builtin_ctzll(__builtin_amdgcn_read_exec()))
      atomicAdd(O.cost + by, dt);
  }
  if constexpr (TILES) {
    // the stream carries the shading terms (shade.h)
    const int tiles_x = (A.width + 7) >> 3;
    const int tile = by * tiles_x + blockIdx.x * kWgWaves + wave;
    store_tiles(A.rgba, tiles_x * ((A.rows + 7) >> 3), tile, lane, valid, c);
    if (tile == 0) store_tiles_shade(A.rgba, frame_shade(A), lane);
  } else if constexpr (SSAA) {
    // every lane's colour, the group sums in the contract's tree order, and
    // the group's (0, 0) lane scales by 1 / S^2 (a power of two: one
    // rounding, denormals kept), converts and writes the output pixel
    float4 s = c;
    if constexpr (!LIGHTS) s = shade_colour<SDF_EXACT>(frame_shade(A), c.x, c.y, c.z);
    const int lg = A.ss_log2;
    const bool four = lg == 2;
    const float sx = ssaa_sum(s.x, four), sy = ssaa_sum(s.y, four), sz = ssaa_sum(s.z, four);
    const int sub = (1 << lg) - 1;
    if ((lane & sub) == 0 && ((lane >> 3) & sub) == 0) {
      const float w = four ? 0.0625f : 0.25f;
      const size_t oo = (size_t)((A.frame_rows ? y : pr) >> lg) * A.out_width + (x >> lg);
      store_pixel(A.format, A.rgba, oo, make_float4(sx * w, sy * w, sz * w, 1.0f));
    }
  } else if constexpr (LIGHTS) {
    store_pixel(A.format, A.rgba, o, c);
  } else {
    store_pixel(A.format, A.rgba, o, pixel_value(A, A.format, c));
  }
  if constexpr (STEPS) {
    if (A.steps && valid) reinterpret_cast<int2*>(A.steps)[o] = make_int2(sp, ss);
  }
}

template <class Scene, bool TILES, bool STEPS>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_WAVES_PER_EU, SDF_WAVES_PER_EU)))
void render(RenderArgs args) {
  (void)args;
  render_body<Scene, false, STEPS>();
}
// the TILES instantiation at the plain kernel's occupancy (8 waves per SIMD):
// its encoder epilogue would otherwise hold it to 7
template <class Scene, bool TILES, bool STEPS>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_WAVES_PER_EU, SDF_WAVES_PER_EU)))
void render_tiles(RenderArgs args) {
  (void)args;
  render_body<Scene, true, STEPS>();
}
// the supersampling instantiation (sdf_params.samples = 2 or 4, a uniform
// read from the arguments): the plain kernel's pixels as sub-samples, with
// the resolve epilogue; with and without step recording like `render`, so a
// sub-sample is bit for bit the pixel the plain kernel of the same STEPS
// writes for the S W x S H frame
template <class Scene, bool STEPS>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_WAVES_PER_EU, SDF_WAVES_PER_EU)))
void render_ssaa(RenderArgs args) {
  (void)args;
  render_body<Scene, false, STEPS, true>();
}

// the multi-light instantiations (sdf_render_lights; the count and the colour
// flag are uniforms), with and without step recording and the supersampling
// resolve.  P, N, ao, the channel sums and a copy of the culling state live
// across the loop over the lights on top of a shadow march's registers, so
// these kernels take an occupancy of their own (DESIGN.md, Lights)
// (CSG8: 79 VGPRs fast, which 6 waves per SIMD hold; exact spilled 32 bytes
// per lane there and takes 5)
#ifndef SDF_LIGHTS_WAVES_PER_EU
#define SDF_LIGHTS_WAVES_PER_EU (SDF_EXACT ? 5 : 6)
#endif
template <class Scene, bool STEPS, bool SSAA>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_LIGHTS_WAVES_PER_EU, SDF_LIGHTS_WAVES_PER_EU)))
void render_lights(RenderArgs args) {
  (void)args;
  render_body<Scene, false, STEPS, SSAA, true>();
}

// the per-primitive material instantiations (sdf_render_materials): the
// lights kernels with the material fold at P between the surface and the
// lights (shade_pixel_materials); the fold's nine running components are dead
// before the first shadow march, where the blended dif and ref (6 VGPRs) stay
// live instead of uniform ones (DESIGN.md, Materials: the register figures
// and the choice of occupancy)
// (CSG8 exact: 96 VGPRs at the lights kernels' 5 waves per SIMD, no scratch.
// CSG8 fast at their 6 waves: 80 VGPRs and 20-28 bytes of scratch per lane,
// stored once before the loop over the lights and read back after it, one
// dword per light inside it, none in a march; at 5 waves 87-90 VGPRs without
// scratch, measured slower by about half a percent (1 light) and one percent
// (4 lights) on C4 at 1080p (profiles/materials_C4.json, materials_w5), so 6
// stays)
#ifndef SDF_MATERIALS_WAVES_PER_EU
#define SDF_MATERIALS_WAVES_PER_EU SDF_LIGHTS_WAVES_PER_EU
#endif
template <class Scene, bool STEPS, bool SSAA>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_MATERIALS_WAVES_PER_EU, SDF_MATERIALS_WAVES_PER_EU)))
void render_materials(RenderArgs args) {
  (void)args;
  render_body<Scene, false, STEPS, SSAA, true, true>();
}

// the reflect instantiations (sdf_render_reflect): the materials kernels'
// pixel inside a loop over the path's layers (shade_pixel_reflect).  The next
// ray, the weights, the composite and the step sums live across a whole layer
// on top of the materials kernel's registers, so these kernels take an
// occupancy of their own (DESIGN.md, Reflections: the register figures)
#ifndef SDF_REFLECT_WAVES_PER_EU
#define SDF_REFLECT_WAVES_PER_EU 4
#endif
template <class Scene, bool STEPS, bool SSAA, bool FOLD>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_REFLECT_WAVES_PER_EU, SDF_REFLECT_WAVES_PER_EU)))
void render_reflect(RenderArgs args) {
  (void)args;
  render_body<Scene, false, STEPS, SSAA, true, FOLD, true>();
}

// the env instantiations (sdf_render_env): the reflect kernels' path with the
// miss test between a layer's march and its surface work (shade_pixel_env),
// at the reflect kernels' occupancy (DESIGN.md, Environment: the register
// figures)
#ifndef SDF_ENV_WAVES_PER_EU
#define SDF_ENV_WAVES_PER_EU SDF_REFLECT_WAVES_PER_EU
#endif
template <class Scene, bool STEPS, bool SSAA, bool FOLD>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_ENV_WAVES_PER_EU, SDF_ENV_WAVES_PER_EU)))
void render_env(RenderArgs args) {
  (void)args;
  render_body<Scene, false, STEPS, SSAA, true, FOLD, true, true>();
}

// The persistent frame-sequence kernel (sdf_render_frames): every wave
// builds its scene registers once, then renders 8x8 tiles (item = frame *
// tiles_per_frame + tile, row-major), `chunk` consecutive items per
// request to its workgroup's work queue; queue q hands out the chunks q,
// q + queues, q + 2 queues, ...  A wave asks for its next chunk while it
// renders the current one, and ends on the first chunk past the end, so the
// grid drains whatever its size (every queue has at least one workgroup).
// A tile's pixels come from the same shade_pixel as sdf_render's: identical
// frames.
template <bool STEPS, class Scene>
__device__ __forceinline__ void frames_tile(KA& A, const KARG FramesArgs& FA, const Scene& scene,
                                            uint32_t item, int lane) {
  const uint32_t per_frame = (uint32_t)FA.tiles_per_frame;
  const uint32_t f = item / per_frame;
  const uint32_t t = item - f * per_frame;
  const uint32_t ty = t / (uint32_t)FA.tiles_x;
  const int x = (int)(t - ty * (uint32_t)FA.tiles_x) * 8 + (lane & 7);
  const int y = (int)ty * 8 + (lane >> 3);
  if (x < A.width && y < A.height) {
    const FrameView V{FA.frame[f]};
    int sp = 0, ss = 0;
    const float4 c = shade_pixel<STEPS>(A, scene, V, x, y, sp, ss);
    const size_t o = (size_t)y * A.width + x;
    store_pixel(A.format, V.rgba(), o, pixel_value(A, A.format, c));
    if constexpr (STEPS) {
      if (V.steps()) reinterpret_cast<int2*>(V.steps())[o] = make_int2(sp, ss);
    }
  }
}

// the persistent frames kernel's occupancy: its queue state on top of the
// pixel's (CSG8 exact at 8 waves/SIMD spilled 156-160 bytes per lane)
#ifndef SDF_FRAMES_WAVES_PER_EU
#define SDF_FRAMES_WAVES_PER_EU SDF_WAVES_PER_EU
#endif
template <class Scene, bool STEPS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SDF_FRAMES_WAVES_PER_EU, SDF_FRAMES_WAVES_PER_EU)))
void render_frames(FramesArgs args) {
  (void)args;
  const KARG FramesArgs& FA = *(const KARG FramesArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
  KA& A = FA.a;
  const int lane = threadIdx.x & 63;
  const Scene scene(A);
  const uint32_t total = (uint32_t)FA.nframes * (uint32_t)FA.tiles_per_frame;
  if (FA.schedule == 1) {
    // static: wave w takes items w, w + W, w + 2 W, ... (W waves in the grid)
    const uint32_t W = gridDim.x * (blockDim.x >> 6);
    for (uint32_t item = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); item < total;
         item += W)
      frames_tile<STEPS>(A, FA, scene, __builtin_amdgcn_readfirstlane(item), lane);
    return;
  }
  const uint32_t nq = (uint32_t)FA.queues;
  const uint32_t q = blockIdx.x % nq;
  uint32_t* const counter = FA.counter + q * kQueueStride;
  const uint32_t ck = (uint32_t)FA.chunk;
  const uint32_t chunks = (total + ck - 1) / ck;
  uint32_t next = 0u;
  if (lane == 0) next = atomicAdd(counter, 1u);
  for (;;) {
    const uint32_t chunk = __builtin_amdgcn_readfirstlane(next) * nq + q;
    if (chunk >= chunks) break;
    if (lane == 0) next = atomicAdd(counter, 1u);
#pragma unroll 1
    for (uint32_t i = chunk * ck; i < chunk * ck + ck && i < total; ++i)
      frames_tile<STEPS>(A, FA, scene, i, lane);
  }
}

// ---- queries (sdf_abi.h "Queries": sdf_trace, sdf_trace_camera, sdf_sample) --
// What the render kernels compute on the way to a colour, written out: the
// primary march's distance and iteration count, and at the point it ends on
// the normal and the primitive that owns the surface.  The march, the normal
// and the scene value are trace_march, trace_surface, trace_shape and
// Scene::eval as the render kernels call them; only the owner fold
// (owner_step) is the queries' own.  The uniforms ride in a QueryArgs of
// their own (kernel_args.h): the scene evaluators read its KernelArgs at the
// start of the kernel-argument segment, as in a render.  Which outputs are
// written is a uniform branch on their pointers: one kernel per scene, kind
// and precision serves every selection.  No address depends on ray data, and
// every loop is bounded by max_steps: a ray outside the working range gives
// unspecified values, never a fault or a hang.
//
// What follows a query ray's march (S: its end, sp: its count, i: its entry).
// A miss (d > max_dist, the comparison that ends a reflect path; a NaN d is
// none) evaluates nothing more: normal (0, 0, 0), owner -1 -- behind a real
// branch, as a missed layer under a sky (env_layer).
template <class Scene>
__device__ __forceinline__ void query_store(KA& A, const KARG QueryArgs& Q, const Scene& scene,
                                            MarchState& mst, Surface& S, int sp, size_t i) {
  if (Q.t) Q.t[i] = S.d;
  if (Q.steps) Q.steps[i] = sp;
  const bool want_n = Q.normal != nullptr, want_w = Q.prim != nullptr;
  if (!want_n && !want_w) return;
  V3 N = mk(0.0f, 0.0f, 0.0f);
  int w = -1;
  if (!(S.d > A.max_dist)) {
    if (want_w) w = scene.owner_fold(S.P);
    if (want_n) {
      trace_shape(A, scene, mst, S);
      N = S.N;
    }
  }
  if (want_n) {
    float* const o = Q.normal + 3 * i;
    o[0] = N.x;
    o[1] = N.y;
    o[2] = N.z;
  }
  if (want_w) Q.prim[i] = w;
}

// ---- a ray whose direction has no finite length (sdf_abi.h "Queries") ---------
// normalize gives such a direction NaN components (0 / 0, INF / INF), and the
// ray then marches "as the arithmetic says" -- the arithmetic of the scene spec,
// whose min, max and clamp are the GLSL selects (y < x ? y : x, x < y ? y : x):
// a select drops or keeps a NaN operand by its position.  The scene evaluators
// above are built for sdf_validate's working range, where no NaN occurs, and
// take hardware minima and maxima, a clamped FMA and the first primitive's
// value for min(INF, v) there; on a NaN point they give other values.  So a
// lane with such a direction takes this path instead: the scene spec restated
// with the selects, operation for operation the CPU oracle's (oracle_core.h
// scene_sdf, raymarch, normal_central / normal_tetra) over the prepared
// primitive blocks, whose derived values are the oracle's own fp32 results
// (sdf_abi.cpp prepare_prims; k = 4 (k/4) exactly).  A cold path: a wave enters
// it only when one of its lanes has such a direction, and nothing in it is
// tuned.  Primitive scenes only: the Mandelbulb's evaluator has no hardware
// minimum on the way and marches a NaN point as the oracle does.
__device__ __forceinline__ float sel_min(float x, float y) { return y < x ? y : x; }
__device__ __forceinline__ float sel_max(float x, float y) { return x < y ? y : x; }
__device__ __forceinline__ float sel_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ float sel_length(V3 a) { return sel_sqrt(dot(a, a)); }
__device__ __forceinline__ V3 sel_normalize(V3 a) {
  const float l = sel_length(a);
  return mk(a.x / l, a.y / l, a.z / l);
}
__device__ __forceinline__ float sel_box(V3 v, float bx, float by, float bz) {
  const float qx = fabsf(v.x) - bx, qy = fabsf(v.y) - by, qz = fabsf(v.z) - bz;
  const float outside = sel_length(mk(sel_max(qx, 0.0f), sel_max(qy, 0.0f), sel_max(qz, 0.0f)));
  const float inside = sel_min(sel_max(qx, sel_max(qy, qz)), 0.0f);
  return outside + inside;
}
__device__ __forceinline__ float sel_prim(int kind, V3 p, KF q) {
  const V3 v = sub(p, mk(q[0], q[1], q[2]));
  switch (kind) {
    case SDF_PRIM_SPHERE: return sel_length(v) - q[3];
    case SDF_PRIM_PLANE: return dot(p, mk(q[0], q[1], q[2])) + q[3];
    case SDF_PRIM_BOX: return sel_box(v, q[3], q[4], q[5]);
    case SDF_PRIM_ROUND_BOX: return sel_box(v, q[3], q[4], q[5]) - q[6];
    case SDF_PRIM_TORUS: {
      const float qx = sel_sqrt(v.x * v.x + v.z * v.z) - q[3];
      return sel_sqrt(qx * qx + v.y * v.y) - q[4];
    }
    case SDF_PRIM_CAPSULE: {
      const V3 ba = mk(q[3], q[4], q[5]);
      const float h = sel_min(sel_max(dot(v, ba) / q[7], 0.0f), 1.0f);
      return sel_length(sub(v, muls(ba, h))) - q[6];
    }
    default: {
      const float dx = sel_sqrt(v.x * v.x + v.z * v.z) - q[3];
      const float dy = fabsf(v.y) - q[4];
      const float inside = sel_min(sel_max(dx, dy), 0.0f);
      const float ox = sel_max(dx, 0.0f), oy = sel_max(dy, 0.0f);
      return inside + sel_sqrt(ox * ox + oy * oy);
    }
  }
}
__device__ __forceinline__ float sel_smin(float a, float b, float k) {
  const float h = sel_max(k - fabsf(a - b), 0.0f) / k;
  return sel_min(a, b) - h * h * k * 0.25f;
}
__device__ __forceinline__ float sel_combine(int op, float d, float v, float k) {
  switch (op) {
    case SDF_OP_UNION: return sel_min(d, v);
    case SDF_OP_SMOOTH_UNION: return sel_smin(d, v, k);
    case SDF_OP_SUBTRACT: return sel_max(d, -v);
    case SDF_OP_INTERSECT: return sel_max(d, v);
    case SDF_OP_SMOOTH_SUBTRACT: return -sel_smin(-d, v, k);
    default: return -sel_smin(-d, -v, k);
  }
}
// the scene value at p, and (OWNER) the owner fold's primitive beside it
template <bool OWNER>
__device__ __forceinline__ float sel_scene(KA& A, V3 p, int& w) {
  float d = INFINITY;
  const int n = A.prim_count;
#pragma unroll 1
  for (int i = 0; i < n; i++) {
    const KARG sdf_primitive& pr = A.prims[i];
    const float v = sel_prim(pr.kind, p, pr.p);
    if constexpr (OWNER) {
      if (owner_step(pr.op, d, v)) w = i;
    }
    d = sel_combine(pr.op, d, v, 4.0f * SMIN_K(pr));
  }
  return d;
}
__device__ __forceinline__ float sel_scene(KA& A, V3 p) {
  int w = 0;
  return sel_scene<false>(A, p, w);
}
// the whole query of one such ray, stored as query_store stores it
__device__ __forceinline__ void sel_query(KA& A, const KARG QueryArgs& Q, V3 O, V3 D, size_t i) {
  float d = 0.0f;
  int sp = 0;
#pragma unroll 1
  for (; sp < A.max_steps;) {
    const float s = sel_scene(A, add(O, muls(D, d)));
    d += s;
    sp++;
    if (d > A.max_dist || s < A.eps) break;
  }
  if (Q.t) Q.t[i] = d;
  if (Q.steps) Q.steps[i] = sp;
  if (!Q.normal && !Q.prim) return;
  V3 N = mk(0.0f, 0.0f, 0.0f);
  int w = -1;
  if (!(d > A.max_dist)) {
    const V3 P = add(O, muls(D, d));
    if (Q.prim) {
      w = 0;
      (void)sel_scene<true>(A, P, w);
    }
    if (Q.normal) {
      const float h = A.normal_eps;
      if (A.normal_mode == SDF_NORMAL_TETRA) {
        const float f0 = sel_scene(A, mk(P.x + h, P.y - h, P.z - h));
        const float f1 = sel_scene(A, mk(P.x - h, P.y - h, P.z + h));
        const float f2 = sel_scene(A, mk(P.x - h, P.y + h, P.z - h));
        const float f3 = sel_scene(A, mk(P.x + h, P.y + h, P.z + h));
        N = sel_normalize(mk(f0 - f1 - f2 + f3, -f0 - f1 + f2 + f3, -f0 + f1 - f2 + f3));
      } else {
        const float nx = sel_scene(A, mk(P.x + h, P.y, P.z)) - sel_scene(A, mk(P.x - h, P.y, P.z));
        const float ny = sel_scene(A, mk(P.x, P.y + h, P.z)) - sel_scene(A, mk(P.x, P.y - h, P.z));
        const float nz = sel_scene(A, mk(P.x, P.y, P.z + h)) - sel_scene(A, mk(P.x, P.y, P.z - h));
        N = sel_normalize(mk(nx, ny, nz));
      }
    }
  }
  if (Q.normal) {
    float* const o = Q.normal + 3 * i;
    o[0] = N.x;
    o[1] = N.y;
    o[2] = N.z;
  }
  if (Q.prim) Q.prim[i] = w;
}

// KIND kQueryRays: lane = ray i of the buffers, a wave 64 consecutive rays
// (the 12-byte-stride dword loads and stores of a wave cover one contiguous
// 768-byte span); O as given, D = normalize(dirs[i]) in the precision's own
// form -- the cached-gap culling is proven for |D| <= 1 + 2^-22 (kPathScale).
// KIND kQueryCamera: lane = pixel (x, y), waves are the render kernels' 8x8
// tiles and the ray is trace_surface's, so the march is the render's.
// KIND kQueryPoints: lane = point i; the scene value by Scene::eval (no path
// state), the normal from a fresh culling state at path length 0.
// A ragged last wave (tile) leaves with its lanes beyond n (the frame) idle.
template <class Scene, int KIND>
__device__ __forceinline__ void query_body() {
  const KARG QueryArgs& Q = *(const KARG QueryArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = Q.a;
  if constexpr (KIND == kQueryCamera) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int x = blockIdx.x * (8 * kWgWaves) + wave * 8 + (lane & 7);
    const int y = blockIdx.y * 8 + (lane >> 3);
    if (x >= A.width || y >= A.height) return;
    const Scene scene(A);
    MarchState mst;
    Surface S;
    int sp = 0;
    trace_surface<Scene, ArgsView, false>(A, scene, ArgsView{A}, x, y, sp, mst, S);
    query_store(A, Q, scene, mst, S, sp, (size_t)y * A.width + x);
  } else {
    const long long i = (long long)blockIdx.x * (64 * kWgWaves) + threadIdx.x;
    if (i >= Q.n) return;
    const Scene scene(A);
    const float* const o = Q.in0 + 3 * i;
    const V3 O = mk(o[0], o[1], o[2]);
    if constexpr (KIND == kQueryRays) {
      const float* const r = Q.in1 + 3 * i;
      const V3 D = normalize(mk(r[0], r[1], r[2]));
      // a direction without a finite length (D has a NaN or INF component):
      // the scene spec's own arithmetic (sel_query), and the lane is done
      const bool odd = !(fabsf(D.x) < INFINITY && fabsf(D.y) < INFINITY && fabsf(D.z) < INFINITY);
      if (A.scene_kind == SDF_SCENE_PRIMITIVES && __builtin_amdgcn_ballot_w64(odd) != 0) {
        asm volatile("" ::: "memory");   // a real branch: never if-converted into the march
        if (odd) {
          sel_query(A, Q, O, D, (size_t)i);
          return;
        }
      }
      MarchState mst;
      Surface S;
      int sp = 0;
      trace_march(A, scene, O, D, sp, mst, S);
      S.cam = O;
      S.ray = D;
      query_store(A, Q, scene, mst, S, sp, (size_t)i);
    } else {
      if (Q.t) Q.t[i] = scene.eval(O);
      if (Q.normal) {
        MarchState mst;
        Surface S;
        S.P = O;
        S.tP = 0.0f;
        trace_shape(A, scene, mst, S);
        float* const q = Q.normal + 3 * i;
        q[0] = S.N.x;
        q[1] = S.N.y;
        q[2] = S.N.z;
      }
    }
  }
}

// the query kernels' occupancy: a march, the normal's taps and the owner fold
// (no shadow march, no colour)
#ifndef SDF_QUERY_WAVES_PER_EU
#define SDF_QUERY_WAVES_PER_EU SDF_WAVES_PER_EU
#endif
template <class Scene, int KIND>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_QUERY_WAVES_PER_EU, SDF_QUERY_WAVES_PER_EU)))
void query(QueryArgs args) {
  (void)args;
  query_body<Scene, KIND>();
}

// ---- gradients (sdf_abi.h "Gradients": sdf_sample_grad) -------------------------
#if !SDF_TU_BULB
#include "grad_kernel.inc"
#endif

// ---- isosurface meshes (sdf_abi.h "Meshes": sdf_mesh_count, sdf_mesh_emit;
// "Sharp meshes": sdf_mesh_emit_sharp, over the gradient's functions) -------------
#include "mesh_kernel.inc"

// ---- caller-supplied rays (sdf_abi.h "Rays": sdf_render_rays, sdf_camera_rays) --
// The path of shade_pixel_reflect (ENV: shade_pixel_env) whose layer 0 is read
// from memory instead of being formed from (x, y): every layer, the first
// included, is what those functions' loops run for j >= 1 -- trace_ray_path and
// surface_colour, or trace_march_path and env_layer, the very device functions --
// from the lane's own eye.  In exact precision nothing is contracted, so the
// ray of a pixel gives the pixel's bits (tests/test_gpu_rays.py holds them).
template <bool STEPS, bool FOLD, bool ENV, class Scene, class View>
__device__ __forceinline__ float4 shade_ray(KA& A, const KARG LightsArgs& L,
                                            const KARG MaterialArgs& M,
                                            const KARG ReflectArgs& R, const KARG EnvArgs& E,
                                            const Scene& scene, const View& V, const V3 O,
                                            const V3 D, int& sp, int& ss) {
  ReflectPath path;
  path.O = O;
  path.D = D;
#pragma unroll 1
  for (int j = 0; path.live; j++) {
    MarchState mst;
    Surface S;
    int spj = 0;
    if constexpr (ENV) {
      trace_march_path(A, scene, path.O, path.D, spj, mst, S);
      S.cam = path.O;
      S.ray = path.D;
      env_layer<STEPS, FOLD>(A, L, M, R, E, scene, V, j, S, mst, spj, path);
    } else {
      int ssj = 0;
      trace_ray_path(A, scene, path.O, path.D, spj, mst, S);
      float C[3], mr[3];
      surface_colour<STEPS, FOLD>(A, L, M, scene, V, S, mst, ssj, C, mr);
      path.layer_done(A, R, j, S, C, mr, spj, ssj);
    }
  }
  sp = path.sp;
  ss = path.ss;
  return make_float4(path.acc[0], path.acc[1], path.acc[2], 1.0f);
}

// lane = ray i of the buffers, a wave 64 consecutive rays, loaded as query_body
// loads them; O as given, D = dirs[i] under SDF_RAYS_UNIT (a uniform), else its
// normalize in the precision's own form.  A ray whose D has a component that
// is not finite is inactive: it stores its zeros and leaves through a real
// branch, never if-converted into the march.  A ragged last wave leaves with
// its lanes beyond n idle.  No address depends on ray data.
template <class Scene, bool STEPS, bool FOLD, bool ENV>
__device__ __forceinline__ void rays_body() {
  const KARG char* const seg = (const KARG char*)__builtin_amdgcn_kernarg_segment_ptr();
  const KARG RaysArgs& Q = *(const KARG RaysArgs*)seg;
  KA& A = Q.a;
  const long long i = (long long)blockIdx.x * (64 * kWgWaves) + threadIdx.x;
  if (i >= Q.n) return;
  const float* const o = Q.in0 + 3 * i;
  const V3 O = mk(o[0], o[1], o[2]);
  const float* const r = Q.in1 + 3 * i;
  V3 D = mk(r[0], r[1], r[2]);
  if (!(Q.flags & SDF_RAYS_UNIT)) D = normalize(D);
  const bool odd = !(fabsf(D.x) < INFINITY && fabsf(D.y) < INFINITY && fabsf(D.z) < INFINITY);
  if (__builtin_amdgcn_ballot_w64(odd) != 0) {
    asm volatile("" ::: "memory");   // a real branch: never if-converted into the march
    if (odd) {
      store_pixel(A.format, A.rgba, (size_t)i, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
      if constexpr (STEPS) {
        if (A.steps) reinterpret_cast<int2*>(A.steps)[i] = make_int2(0, 0);
      }
      return;
    }
  }
  const Scene scene(A);
  const KARG LightsArgs& L = *(const KARG LightsArgs*)(seg + __builtin_offsetof(RaysArgs, l));
  const KARG MaterialArgs& M = *(const KARG MaterialArgs*)(seg + __builtin_offsetof(RaysArgs, m));
  const KARG ReflectArgs& R = *(const KARG ReflectArgs*)(seg + __builtin_offsetof(RaysArgs, r));
  const KARG EnvArgs& E = *(const KARG EnvArgs*)(seg + __builtin_offsetof(RaysArgs, e));
  int sp = 0, ss = 0;
  const float4 c = shade_ray<STEPS, FOLD, ENV>(A, L, M, R, E, scene, ArgsView{A}, O, D, sp, ss);
  store_pixel(A.format, A.rgba, (size_t)i, c);
  if constexpr (STEPS) {
    if (A.steps) reinterpret_cast<int2*>(A.steps)[i] = make_int2(sp, ss);
  }
}

// the rays instantiations (sdf_render_rays), with and without step recording:
// render_rays runs the reflect kernels' layers, render_rays_env the env
// kernels', at the env kernels' occupancy (DESIGN.md, render_rays: the
// register figures)
#ifndef SDF_RAYS_WAVES_PER_EU
#define SDF_RAYS_WAVES_PER_EU SDF_ENV_WAVES_PER_EU
#endif
template <class Scene, bool STEPS, bool FOLD>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_RAYS_WAVES_PER_EU, SDF_RAYS_WAVES_PER_EU)))
void render_rays(RaysArgs args) {
  (void)args;
  rays_body<Scene, STEPS, FOLD, false>();
}
template <class Scene, bool STEPS, bool FOLD>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_RAYS_WAVES_PER_EU, SDF_RAYS_WAVES_PER_EU)))
void render_rays_env(RaysArgs args) {
  (void)args;
  rays_body<Scene, STEPS, FOLD, true>();
}

// ---- shading at caller-supplied points (sdf_abi.h "Points": sdf_shade_points) ---
// The materials pipeline entered at a point instead of behind a primary march:
// the Surface {P, N, ao} is built from memory and the normal's taps, then
// surface_colour -- the very fold and light loop of the reflect layers, with the
// eye in S.cam -- gives the colour, and its hook hands out what a render keeps
// to itself.  The view light_terms takes tells it only whether every shadow
// march runs to the reference's break (STEPS: `shadow` or `steps` asked for).
struct PointsView {
  const void* full;   // non-null: they do
  __device__ __forceinline__ const void* steps() const { return full; }
};
// Whether the fold and the loop run and whether there is an eye (uniforms), and
// where the lane's point has its material, shadow factors and counts stored.
struct PointsHook {
  static constexpr bool kOn = true;
  bool want_fold, want_lights, want_eye;
  float* material_out;   // the point's 9 components, or null
  float* shadow_out;     // the point's L.n factors, or null
  int32_t* steps_out;    // the point's L.n counts, or null
  mutable float sh = 1.0f;
  __device__ __forceinline__ bool fold() const { return want_fold; }
  __device__ __forceinline__ void material(const float (&m)[9]) const {
    if (material_out) {
#pragma unroll
      for (int c = 0; c < 9; c++) material_out[c] = m[c];
    }
  }
  __device__ __forceinline__ bool lights() const { return want_lights; }
  __device__ __forceinline__ bool eye() const { return want_eye; }
  __device__ __forceinline__ void shadow(float s) const { sh = s; }
  __device__ __forceinline__ void light(int i, int count) const {
    if (shadow_out) shadow_out[i] = sh;
    if (steps_out) steps_out[i] = count;
  }
};

// lane = point i of the buffers, a wave 64 consecutive points, loaded as
// rays_body loads its rays (3 dwords per lane at stride 12: a wave's loads and
// stores cover one contiguous span).  Every decision on what is evaluated is a
// uniform of the argument block.  A ragged last wave leaves with its lanes
// beyond n idle, as there.  No address or loop bound depends on point data.
template <class Scene, bool STEPS, bool FOLD>
__device__ __forceinline__ void points_body() {
  const KARG char* const seg = (const KARG char*)__builtin_amdgcn_kernarg_segment_ptr();
  const KARG PointsArgs& Q = *(const KARG PointsArgs*)seg;
  KA& A = Q.a;
  const long long i = (long long)blockIdx.x * (64 * kWgWaves) + threadIdx.x;
  if (i >= Q.n) return;
  const Scene scene(A);
  const KARG LightsArgs& L = *(const KARG LightsArgs*)(seg + __builtin_offsetof(PointsArgs, l));
  const KARG MaterialArgs& M = *(const KARG MaterialArgs*)(seg + __builtin_offsetof(PointsArgs, m));
  const bool want_rgba = Q.rgba != nullptr;
  const bool want_lights = want_rgba || Q.shadow != nullptr || Q.steps != nullptr;
  const bool want_fold = want_rgba || Q.material != nullptr;
  // the occlusion taps run only when an output needs them (the host zeroes
  // a.ao_taps otherwise)
  const bool want_ao = (A.flags & SDF_FLAG_AO) && A.ao_taps > 0;
  const float lift = Q.lift;

  const float* const q = Q.points + 3 * i;
  MarchState mst;
  Surface S;
  S.P = mk(q[0], q[1], q[2]);
  S.tP = 0.0f;   // a fresh culling state at path length 0, as sdf_sample's normal has
  S.N = mk(0.0f, 0.0f, 0.0f);
  if (Q.normals) {
    const float* const nn = Q.normals + 3 * i;
    S.N = mk(nn[0], nn[1], nn[2]);
  } else if (want_lights || want_ao || lift != 0.0f) {
    trace_shape<Scene, true, false>(A, scene, mst, S);
  }
  if (lift != 0.0f) {
    // P = Q + N lift; the culling state of the taps at Q is not one of P
    S.P = mk(S.P.x + S.N.x * lift, S.P.y + S.N.y * lift, S.P.z + S.N.z * lift);
    mst = MarchState();
  }
  trace_shape<Scene, false, true>(A, scene, mst, S);
  S.cam = mk(Q.eye[0], Q.eye[1], Q.eye[2]);
  S.ray = mk(0.0f, 0.0f, 0.0f);
  S.d = 0.0f;
  if (Q.ao) Q.ao[i] = S.ao;
  if (!want_lights && !want_fold) return;

  PointsHook hook{want_fold, want_lights, want_rgba && (Q.flags & SDF_POINTS_EYE) != 0,
                  Q.material ? Q.material + 9 * i : nullptr,
                  Q.shadow ? Q.shadow + (long long)L.n * i : nullptr,
                  Q.steps ? Q.steps + (long long)L.n * i : nullptr};
  float C[3], mr[3];
  int ss = 0;
  const PointsView V{Q.steps ? (const void*)Q.steps : (const void*)Q.shadow};
  surface_colour<STEPS, FOLD>(A, L, M, scene, V, S, mst, ss, C, mr, &hook);
  if constexpr (!FOLD) {
    // a Mandelbulb: the one material of the launch
    if (Q.material) {
      float* const o = Q.material + 9 * i;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        o[c] = A.mat_amb[c];
        o[3 + c] = A.mat_dif[c];
        o[6 + c] = A.mat_ref[c];
      }
    }
  }
  if (want_rgba) reinterpret_cast<float4*>(Q.rgba)[i] = make_float4(C[0], C[1], C[2], 1.0f);
}

// the points instantiations (sdf_shade_points), with every shadow march run to
// the reference's break (STEPS) and without.  No path state lives across the
// light loop, so the registers are the materials kernels': CSG8 exact 96 VGPRs
// at their 5 waves per SIMD; CSG8 fast at their 6 waves 80 VGPRs and 12-28
// bytes of scratch per lane, at 5 waves no scratch, and no points kernel is
// to use scratch, so 5 in both precisions (DESIGN.md, shade_points: the
// register figures)
#ifndef SDF_POINTS_WAVES_PER_EU
#define SDF_POINTS_WAVES_PER_EU 5
#endif
template <class Scene, bool STEPS, bool FOLD>
__global__ __launch_bounds__(64 * kWgWaves) __attribute__((amdgpu_waves_per_eu(SDF_POINTS_WAVES_PER_EU, SDF_POINTS_WAVES_PER_EU)))
void shade_points(PointsArgs args) {
  (void)args;
  points_body<Scene, STEPS, FOLD>();
}

#if !SDF_TU_BULB && !defined(__HIPCC_RTC__)
// sdf_camera_rays: (O_0, D_0) of pixel (x, y), entry y * width + x.  The
// statements are trace_surface's own, restated: lifted out of it into a shared
// function, fast precision contracted the normalisations' sums of squares in
// another order and every fast kernel's rays moved by an ulp (see there), so
// the render kernels keep theirs in place.  Waves are the render's 8x8 tiles;
// either output may be null (a uniform branch).
__global__ __launch_bounds__(64 * kWgWaves)
void camera_rays(RaysArgs args) {
  (void)args;
  const KARG RaysArgs& Q = *(const KARG RaysArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = Q.a;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int x = blockIdx.x * (8 * kWgWaves) + wave * 8 + (lane & 7);
  const int y = blockIdx.y * 8 + (lane >> 3);
  if (x >= A.width || y >= A.height) return;
#if SDF_EXACT
  const float qx = crm::div_refined((float)(2 * x + 1), (float)A.width, A.inv_width) - 1.0f;
  const float qy = crm::div_refined((float)(2 * y + 1), (float)A.height, A.inv_height) - 1.0f;
#else
  const float qx = (float)(2 * x + 1) * A.inv_width - 1.0f;
  const float qy = (float)(2 * y + 1) * A.inv_height - 1.0f;
#endif
  V3 r0 = normalize(mk(qx * A.aspect, qy, A.focal));
  KF m = A.inv_view;
  V3 r1 = mk(m[0] * r0.x + m[4] * r0.y + m[8] * r0.z + m[12] * 0.0f,
             m[1] * r0.x + m[5] * r0.y + m[9] * r0.z + m[13] * 0.0f,
             m[2] * r0.x + m[6] * r0.y + m[10] * r0.z + m[14] * 0.0f);
  const V3 ray = normalize(r1);
  const size_t i = (size_t)y * A.width + x;
  if (Q.out0) {
    float* const q = Q.out0 + 3 * i;
    q[0] = A.cam[0];
    q[1] = A.cam[1];
    q[2] = A.cam[2];
  }
  if (Q.out1) {
    float* const q = Q.out1 + 3 * i;
    q[0] = ray.x;
    q[1] = ray.y;
    q[2] = ray.z;
  }
}
#endif

#undef scene_sdf
#undef DIVK
#undef SMIN_K
#undef SMIN_IK
#undef SMIN_SC
#undef SMIN_KSC

}  // namespace SDF_NS

}  // namespace sdf
