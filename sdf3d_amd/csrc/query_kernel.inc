// query_kernel.inc -- the query family (sdf_trace, sdf_trace_camera, sdf_sample).
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

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
// a query entry, built-in or run-time (jit_entry.inc)
#define SDF_QUERY_KERNEL(name, Scene, KIND)                  \
  SDF_KERNEL(SDF_WG_BOUND, SDF_QUERY_WAVES_PER_EU)          \
  void name(QueryArgs args) {                                \
    (void)args;                                              \
    query_body<Scene, KIND>();                               \
  }
template <class Scene, int KIND>
SDF_QUERY_KERNEL(query, Scene, KIND)
