// host_api.h -- the library's internal host interfaces.  Not installed, host
// only: never handed to hipRTC, no part of sdf_kernel_id.
//
//   RenderPlan: a prepared scene and the kernel that serves it, made by
//     make_render_plan (sdf_abi.cpp); the frame driver (driver.cpp) and
//     sdf_render_multi (multi.cpp) keep plans and re-launch them.
//   The kernel launchers: each render unit's as a RenderUnit, the run-time
//     specialised ones (jit.cpp), and the ladder over both, launch_planned.
//   Per kernel family its grid and its argument contract, which the built-in
//     launchers (render_launch.inc) and the run-time specialised ones share.
//
// A new kernel family is a kernel body (its kernel file beside render_kernel.inc), a
// launch_*_scene (render_launch.inc) with a RenderUnit slot, a *_args_fit and
// *_grid here, and one launch_planned (or launch_built_in) line where its
// entry point has the scene's plan (sdf_abi.cpp scene_plan).
#pragma once

#include "../../include/sdf_abi.h"
#include "kernel_args.h"

namespace sdf {

// One validated, prepared render launch: the kernel arguments of an
// sdf_render call (camera hoisted, primitive blocks and culling bounds
// prepared) plus the kernel that serves it.  Building one costs a few
// microseconds of host time; launching one is the kernel launch alone
// (plus the TILES compaction).  sdf_render builds and launches one per call;
// the frame driver keeps one per buffer set and re-launches it every frame.
struct RenderPlan {
  KernelArgs a;
  int variant;             // built-in variant, or kVariantGeneric
  bool jit;                // a run-time specialised kernel is tried first
  bool exact;
  int sig[SDF_MAX_PRIMS];  // the scene signature (jit)
  int nsig;
  int rows;                // 0: nothing to render
  int tiles_ntiles;        // > 0: TILES output, compacted after the render
  uint32_t* tiles_used = nullptr;   // TILES: also receives the stream's length (device)
  RowOrder order{};        // dispatch order of the 8-row blocks (a Schedule's; n = 0: none)
  LightsArgs lights{};     // sdf_render_lights (n = 0: the one light of `a`)
  MaterialArgs materials{};   // sdf_render_materials (n = 0: the one material of `a`)
  ReflectArgs reflect{};   // sdf_render_reflect (on = 0: one layer, no reflect kernel)
  EnvArgs env{};           // sdf_render_env (on = 0: no sky, no fog, no env kernel)
};

// A render schedule (sdf_schedule): the dispatch order of a plan's 8-row
// blocks from the cost the kernels measured for them in earlier frames.
struct Schedule;
Schedule* schedule_create(int rows, int period);
void schedule_destroy(Schedule* s);
// before a launch: the latest order (once a cost snapshot has landed) into
// plan->order, and the cost buffer the kernel adds to
// SDF_E_HIP when the last cost copy failed (the schedule then measures anew)
int schedule_apply(Schedule* s, RenderPlan* plan);
// after the launch on `stream`: every `period` launches a snapshot of the
// costs is copied to the host, behind the launch
int schedule_after(Schedule* s, void* stream);

// Rows a tiling owns (sdf_owned_rows), or SDF_E_INVALID_ARG.
int count_rows(int height, const sdf_tiling& t);
int tiling_run(const sdf_tiling& t);
int tiling_step(const sdf_tiling& t);
int tiling_gap_rows(const sdf_tiling& t);  // (step - 1) * block_rows

// What every shading call is made of.  A call without a part leaves it null
// (`camera`: rays and points; `reflect`, `env`: none asked) or at one entry
// (`lights`, `materials`: the one light and material of sdf_render).
struct Request {
  const sdf_scene* scene;
  const sdf_camera* camera;
  const sdf_light* lights;
  int32_t nlights, light_flags;
  const sdf_material* materials;
  int32_t nmaterials;
  const sdf_reflect* reflect;
  const sdf_environment* env;
  const sdf_params* params;
  const sdf_tiling* tiling;
};
// How much of a request an entry point takes, and the kernel family that
// serves one (route): each includes the ones before it.
enum Depth { kPlain, kLights, kMaterials, kReflect, kEnv };
// The one validator: every part's rules up to `depth`, once, in the order of
// sdf_abi.h.  `framed`: the call renders a frame through r.camera.
int validate_request(const Request& r, Depth depth, bool framed = true);
// The camera's part alone, for a caller that holds a validated request.
int validate_camera(const sdf_camera* camera);

// Validate and prepare (tiling NULL = the whole frame).  SDF_OK or an SDF_E_*.
int make_render_plan(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* light,
                     const sdf_material* material, const sdf_params* params,
                     const sdf_tiling* tiling, void* rgba, int32_t* steps, RenderPlan* plan);
// Replace the camera of a prepared plan (validated by the caller).
void plan_set_camera(RenderPlan* plan, const sdf_camera* camera);
// Enqueue a prepared plan on `stream`.  SDF_OK or SDF_E_HIP.
int launch_render_plan(const RenderPlan& plan, void* stream);

// ---- compile-time scene variants (kernel_args.h SDF_FIXED_VARIANTS) ---------
// A primitive's kind as the kernels and the signatures have it: a PLANE whose
// normal is exactly (0,1,0) is a kPrimPlaneY.
inline int prim_kind(const sdf_primitive& p) {
  return p.kind == SDF_PRIM_PLANE && p.p[0] == 0.0f && p.p[1] == 1.0f && p.p[2] == 0.0f
             ? kPrimPlaneY
             : p.kind;
}
// Variant for a validated scene (kVariantGeneric when no fixed one matches).
int select_variant(const sdf_scene& scene);
int scene_signature(const sdf_scene& scene, int* sig);

// ---- the kernel launchers ---------------------------------------------------
// Every launcher returns a hipError_t as int.
//
// The launchers of one render translation unit (render_launch.inc), a slot per
// kernel family.  `variant` selects the compile-time scene specialisation.
struct RenderUnit {
  int (*render)(const RenderArgs& a, int variant, void* stream);
  // the persistent frame-sequence kernel on `nblocks` 256-thread workgroups
  int (*frames)(const FramesArgs& a, int variant, void* stream, int nblocks);
  int (*query)(const QueryArgs& q, int variant, void* stream);   // by QueryArgs::kind
  int (*rays)(const RaysArgs& q, int variant, void* stream);     // sdf_render_rays
  int (*mesh)(const MeshArgs& m, int variant, void* stream, int kind);   // a MeshKind
  int (*points)(const PointsArgs& q, int variant, void* stream);   // sdf_shade_points
  int (*measure)(const MeasureArgs& m, int variant, void* stream);   // sdf_measure, by m.owners
  // one kernel each, in the units of the primitive scenes alone (null in the
  // Mandelbulb's): the ray generator of sdf_camera_rays, and the gradient
  // kernel followed by grad_reduce into `grad_prims`
  int (*camera_rays)(const RaysArgs& q, int variant, void* stream);
  int (*grad)(const GradArgs& g, int variant, void* stream, float* grad_prims);
};
// Each precision's units in its namespace: render_{exact,fast}.hip, and the
// Mandelbulb scene's kernels in render_{exact,fast}_bulb.hip, scheduled for
// ILP (sdf3d_amd/build.py).
namespace exact_impl { const RenderUnit& unit(); const RenderUnit& bulb_unit(); }
namespace fast_impl { const RenderUnit& unit(); const RenderUnit& bulb_unit(); }
inline const RenderUnit& render_unit(bool exact, int variant) {
  const bool bulb = variant == kVariantBulb;
  if (exact) return bulb ? exact_impl::bulb_unit() : exact_impl::unit();
  return bulb ? fast_impl::bulb_unit() : fast_impl::unit();
}
// The run-time specialised kernel of a family for the plan's signature and
// precision (jit.cpp); -1 = none, the caller launches the built-in one.
int launch_render_jit(const RenderArgs& a, const RenderPlan& plan, void* stream);
int launch_query_jit(const QueryArgs& q, const RenderPlan& plan, void* stream);
int launch_rays_jit(const RaysArgs& q, const RenderPlan& plan, void* stream);
int launch_mesh_jit(const MeshArgs& m, const RenderPlan& plan, void* stream, int kind);
int launch_points_jit(const PointsArgs& q, const RenderPlan& plan, void* stream);
int launch_measure_jit(const MeasureArgs& m, const RenderPlan& plan, void* stream);
int jit_compiled_count();

// One kernel launch for a prepared scene, through the built-in kernel of the
// plan's precision and variant: `built_in` names the family's slot, `x` is
// what the slot takes behind the stream.  SDF_OK or SDF_E_HIP.
template <class Args, class... X>
int launch_built_in(const RenderPlan& plan, int (*RenderUnit::*built_in)(const Args&, int, void*, X...),
                    const Args& a, void* stream, X... x) {
  const auto launch = render_unit(plan.exact, plan.variant).*built_in;
  // a family the variant's unit has no kernel for is an error
  const int err = launch ? launch(a, plan.variant, stream, x...) : (int)hipErrorInvalidValue;
  return err == hipSuccess ? SDF_OK : SDF_E_HIP;
}
// The same behind the family's run-time specialised kernel, where the plan
// asks for one and there is one.
template <class Args, class... X>
int launch_planned(const RenderPlan& plan, int (*jit)(const Args&, const RenderPlan&, void*, X...),
                   int (*RenderUnit::*built_in)(const Args&, int, void*, X...), const Args& a,
                   void* stream, X... x) {
  if (plan.jit) {
    const int err = jit(a, plan, stream, x...);
    if (err != -1) return err == hipSuccess ? SDF_OK : SDF_E_HIP;
  }
  return launch_built_in(plan, built_in, a, stream, x...);
}

// the scan over the bricks' counts (mesh.hip): offsets per brick into the
// workspace, the totals into counts[0..3] (device)
int launch_mesh_scan(unsigned char* ws, long long nbricks, long long* counts, void* stream);
// the combination of the measure kernel's records (mesh.hip): `rows` rows into
// moments, the bricks' counts into counts[0..3] (device)
int launch_measure_reduce(const long long* ws, int nblocks, int rows, long long nbricks,
                          long long* moments, long long* counts, void* stream);
int launch_deinterleave(const void* parts, int nparts, int part_stride_rows, int row_bytes,
                        int height, int block_rows, void* frame, void* stream);
int launch_deinterleave_rgb(const void* parts, int nparts, int part_stride_rows, int width,
                            int height, int block_rows, void* frame, void* stream);
int launch_heatmap(const int32_t* steps, int count, int which, int max_steps, int format,
                   void* out, void* stream);
int launch_tiles_decode(const DecodeParts& d, void* frame, const void* parts, void* stream);
// `used_out` (may be null): a device word that also receives the stream's
// length (header word 0), e.g. one slot of the frame driver's lengths array
// whose slots of consecutive frames are all-gathered in one call.
int launch_tiles_compact(void* stream_buf, int ntiles, void* stream, uint32_t* used_out = nullptr);

// ---- the render kernels' launch geometry and argument contract -------------
// Shared by the built-in launchers of every render unit (render_launch.inc)
// and the run-time specialised one (jit.cpp): each refuses with
// hipErrorInvalidValue what render_args_fit refuses.
inline dim3 render_block() { return dim3(64 * kWgWaves); }
inline dim3 render_grid(const KernelArgs& a) {
  return dim3((a.width + 8 * kWgWaves - 1) / (8 * kWgWaves), (a.rows + 7) / 8);
}
// a row order must be a permutation of exactly the grid's rows (the host
// builds it so, sdf_abi.cpp Schedule); anything else renders in launch order
inline bool order_fits(const RenderArgs& r, dim3 grid) {
  return r.o.n == 0 || (r.o.n == (int)grid.y && r.o.n <= kMaxOrderBlocks);
}
// a stream of shading terms (TILES, SHADE32F) carries one light's and one
// material's terms of one layer: no kernel of several writes one
inline bool is_stream(int32_t format) {
  return format == SDF_FORMAT_TILES || format == SDF_FORMAT_SHADE32F;
}
// several lights: at most SDF_MAX_LIGHTS, and never into a stream
inline bool lights_fit(const RenderArgs& r) {
  return r.l.n == 0 || (r.l.n > 0 && r.l.n <= SDF_MAX_LIGHTS && !is_stream(r.a.format));
}
// a material per primitive: one per primitive of a primitive scene, with
// lights (the materials kernels are lights kernels)
inline bool materials_fit(const RenderArgs& r) {
  return r.m.n == 0 || (r.m.n == r.a.prim_count && r.m.n <= SDF_MAX_PRIMS && r.l.n > 0 &&
                        r.a.scene_kind == SDF_SCENE_PRIMITIVES);
}
// mirror reflections: a lights launch that is no stream (lights_fit), with a
// material per primitive exactly when the scene has a primitive list, and
// uniforms inside the contract's ranges (the loop over the layers trusts them)
inline bool reflect_fit(const RenderArgs& r) {
  if (!r.r.on) return true;
  const bool prims = r.a.scene_kind == SDF_SCENE_PRIMITIVES;
  return r.l.n > 0 && !is_stream(r.a.format) && (prims ? r.m.n == r.a.prim_count && r.m.n > 0 : r.m.n == 0) && r.r.bounces >= 0 &&
         r.r.bounces <= SDF_MAX_BOUNCES && r.r.layer >= -1 && r.r.layer <= r.r.bounces;
}
// an environment: a reflect launch (reflect_fit) with known flags, at least
// one of them, never a glow without a sky, and a fog denominator above 0 (the
// kernels trust them)
inline bool env_fit(const RenderArgs& r) {
  if (!r.e.on) return true;
  const int32_t all = SDF_ENV_SKY | SDF_ENV_SUN | SDF_ENV_FOG;
  return r.r.on && r.e.flags != 0 && (r.e.flags & ~all) == 0 &&
         (!(r.e.flags & SDF_ENV_SUN) || (r.e.flags & SDF_ENV_SKY)) &&
         (!(r.e.flags & SDF_ENV_FOG) || r.e.fog_den > 0.0f);
}
// what a render launch on `grid` may be handed
inline bool render_args_fit(const RenderArgs& r, dim3 grid) {
  return order_fits(r, grid) && lights_fit(r) && materials_fit(r) && reflect_fit(r) && env_fit(r);
}

// ---- the rays kernels' launch geometry and argument contract ----------------
// Shared by the built-in launchers (render_launch.inc launch_rays_scene) and
// the run-time specialised one (jit.cpp launch_rays_jit).  64 rays to a wave;
// sdf_render_rays holds n to 2^30, so the grid fits.
inline dim3 rays_grid(const RaysArgs& q) {
  return dim3((unsigned)((q.n + 64 * kWgWaves - 1) / (64 * kWgWaves)));
}
// what a rays launch may be handed: the rules of a reflect render with (e.on)
// or without an environment, on a list of at most 2^30 rays with buffers
inline bool rays_args_fit(const RaysArgs& q) {
  RenderArgs r{};
  r.a.format = q.a.format;
  r.a.prim_count = q.a.prim_count;
  r.a.scene_kind = q.a.scene_kind;
  r.l.n = q.l.n;
  r.m.n = q.m.n;
  r.r = q.r;
  r.e = q.e;
  return q.n > 0 && q.n <= (1ll << 30) && q.in0 && q.in1 && q.a.rgba && q.r.on &&
         (q.flags & ~SDF_RAYS_UNIT) == 0 && lights_fit(r) && materials_fit(r) && reflect_fit(r) &&
         env_fit(r);
}

// ---- the points kernels' launch geometry and argument contract --------------
// Shared by launch_points_scene and launch_points_jit.  64 points to a wave;
// sdf_shade_points holds n to 2^30, so the grid fits.
inline dim3 points_grid(const PointsArgs& q) {
  return dim3((unsigned)((q.n + 64 * kWgWaves - 1) / (64 * kWgWaves)));
}
// every shadow march runs to the reference's break (the STEPS instantiation)
inline bool points_steps(const PointsArgs& q) { return q.shadow || q.steps; }
// what a points launch may be handed: the lights and the table of a materials
// render (a Mandelbulb: no table), at most 2^30 points with a buffer, an output
inline bool points_args_fit(const PointsArgs& q) {
  RenderArgs r{};
  r.a.format = SDF_FORMAT_RGBA32F;
  r.a.prim_count = q.a.prim_count;
  r.a.scene_kind = q.a.scene_kind;
  r.l.n = q.l.n;
  r.m.n = q.m.n;
  const bool prims = q.a.scene_kind == SDF_SCENE_PRIMITIVES;
  return q.n > 0 && q.n <= (1ll << 30) && q.points &&
         (q.rgba || q.ao || q.shadow || q.material || q.steps) &&
         (q.flags & ~SDF_POINTS_EYE) == 0 && q.l.n > 0 && lights_fit(r) && materials_fit(r) &&
         (prims ? q.m.n == q.a.prim_count && q.m.n > 0 : q.m.n == 0);
}

// ---- the query kernels' launch geometry and argument contract ---------------
// Shared by launch_query_scene and launch_query_jit.  Camera rays on the
// render's 8x8 tiles over width x height; buffer rays and points 64 to a wave,
// at most 2^30 of them (sdf_trace and sdf_sample hold n to that), so the grid
// fits.  An empty grid is a success without a launch.
inline bool query_args_fit(const QueryArgs& q) {
  return q.kind == kQueryCamera ||
         ((q.kind == kQueryRays || q.kind == kQueryPoints) && q.n <= (1ll << 30));
}
inline dim3 query_grid(const QueryArgs& q) {
  if (q.kind == kQueryCamera)
    return dim3((q.a.width + 8 * kWgWaves - 1) / (8 * kWgWaves), (q.a.height + 7) / 8);
  return dim3(q.n > 0 ? (unsigned)((q.n + 64 * kWgWaves - 1) / (64 * kWgWaves)) : 0u);
}

// ---- the mesh kernels' launch geometry and argument contract ----------------
// Shared by launch_mesh_scene and launch_mesh_jit.  One wave per brick: a
// count that fits a grid, and the workspace the kernels write through.
inline bool mesh_args_fit(const MeshArgs& m) {
  return m.nbricks > 0 && m.nbricks <= 0x7fffffffll && m.ws;
}
// the sharp kernel besides: the counts its loops run to, and a primitive list
// for the gradient's fold (no Mandelbulb)
inline bool mesh_sharp_args_fit(const MeshArgs& m) {
  return m.refine >= 0 && m.refine <= 8 && m.iterations >= 0 && m.iterations <= 64 &&
         m.a.scene_kind == SDF_SCENE_PRIMITIVES && m.a.prim_count > 0 &&
         m.a.prim_count <= SDF_MAX_PRIMS;
}
inline dim3 mesh_grid(const MeshArgs& m) { return dim3((unsigned)m.nbricks); }

// ---- the measure kernels' launch geometry and argument contract -------------
// Shared by launch_measure_scene and launch_measure_jit.  Grid-stride, one wave
// per workgroup, a record of the workspace per workgroup: the sizes the
// kernel's index arithmetic and its 64-bit sums are proven for.
inline bool measure_args_fit(const MeasureArgs& m) {
  long long bricks = 1;
  for (int c = 0; c < 3; ++c) {
    if (m.n[c] < 1 || m.n[c] > 65536 || m.nb[c] != (m.n[c] + 7) / 8) return false;
    bricks *= m.nb[c];
  }
  return m.nbricks == bricks && m.ws && (m.owners & ~SDF_MEASURE_OWNERS) == 0;
}
inline dim3 measure_grid(const MeasureArgs& m) { return dim3((unsigned)measure_blocks(m.nbricks)); }

}  // namespace sdf
