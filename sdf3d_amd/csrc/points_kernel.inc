// points_kernel.inc -- the points family (sdf_shade_points).
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

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
// a points entry, built-in or run-time (jit_entry.inc)
#define SDF_POINTS_KERNEL(name, Scene, STEPS, FOLD)          \
  SDF_KERNEL(SDF_WG_BOUND, SDF_POINTS_WAVES_PER_EU)         \
  void name(PointsArgs args) {                               \
    (void)args;                                              \
    points_body<Scene, STEPS, FOLD>();                       \
  }
template <class Scene, bool STEPS, bool FOLD>
SDF_POINTS_KERNEL(shade_points, Scene, STEPS, FOLD)
