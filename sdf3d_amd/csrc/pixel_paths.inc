// pixel_paths.inc -- the pixel paths, one per render family (kept separate on
// purpose, see shade_pixel_lights and shade_pixel_materials): shade_pixel*,
// surface_colour, ReflectPath, env_layer, frame_shade, pixel_value.
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

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
