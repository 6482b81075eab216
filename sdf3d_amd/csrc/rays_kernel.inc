// rays_kernel.inc -- the rays family (sdf_render_rays) and sdf_camera_rays.
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

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
// a rays entry, built-in or run-time (jit_entry.inc)
#define SDF_RAYS_KERNEL(name, Scene, STEPS, FOLD, ENV)       \
  SDF_KERNEL(SDF_WG_BOUND, SDF_RAYS_WAVES_PER_EU)           \
  void name(RaysArgs args) {                                 \
    (void)args;                                              \
    rays_body<Scene, STEPS, FOLD, ENV>();                    \
  }
template <class Scene, bool STEPS, bool FOLD>
SDF_RAYS_KERNEL(render_rays, Scene, STEPS, FOLD, false)
template <class Scene, bool STEPS, bool FOLD>
SDF_RAYS_KERNEL(render_rays_env, Scene, STEPS, FOLD, true)

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
