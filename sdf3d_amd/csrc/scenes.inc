// scenes.inc -- the scene evaluators: the culling state and tests, the tap
// generators, GenericScene, FixedScene, BulbScene.
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

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
