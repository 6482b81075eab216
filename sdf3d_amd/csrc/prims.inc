// prims.inc -- the primitives' distance functions, the smooth minimum, combine,
// the folds' steps, the Mandelbulb map, and the select-based evaluator (sel_*).
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

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

// ---- a ray whose direction has no finite length (sdf_abi.h "Queries") ---------
// (the select-based evaluator: query_kernel.inc sel_query, trace.inc
// trace_march_path)
// normalize gives such a direction NaN components (0 / 0, INF / INF), and the
// ray then marches "as the arithmetic says" -- the arithmetic of the scene spec,
// whose min, max and clamp are the GLSL selects (y < x ? y : x, x < y ? y : x):
// a select drops or keeps a NaN operand by its position.  The scene evaluators
// (scenes.inc) are built for sdf_validate's working range, where no NaN occurs, and
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
