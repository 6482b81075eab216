// trace.inc -- a ray's way to a surface and one light's terms there: the views,
// Surface, trace_*, light_terms.
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

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
// do not keep on a NaN point (see query_kernel.inc sel_query: sdf_trace's rays
// of this kind).  So a lane with such a ray takes its primary march through
// prims.inc sel_scene, operation for operation the CPU oracle's raymarch: d_j,
// P_j and the primary step count are the oracle's.  Its culling state stays the
// fresh one.  A cold path behind a real branch, entered by a wave only when one
// of its lanes has such a ray; primitive scenes only, as there.
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
