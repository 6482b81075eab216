// host_api.h -- library-internal host interfaces shared by the C-ABI
// (sdf_abi.cpp) and the native frame driver (driver.cpp).  Not installed.
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

// Validate and prepare (tiling NULL = the whole frame).  SDF_OK or an SDF_E_*.
int make_render_plan(const sdf_scene* scene, const sdf_camera* camera, const sdf_light* light,
                     const sdf_material* material, const sdf_params* params,
                     const sdf_tiling* tiling, void* rgba, int32_t* steps, RenderPlan* plan);
// Replace the camera of a prepared plan (validated by the caller).
void plan_set_camera(RenderPlan* plan, const sdf_camera* camera);
// Enqueue a prepared plan on `stream`.  SDF_OK or SDF_E_HIP.
int launch_render_plan(const RenderPlan& plan, void* stream);

// ---- the render kernels' launch geometry and argument contract -------------
// Shared by the built-in launchers of every render unit (render_kernel.inc)
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
// several lights: at most SDF_MAX_LIGHTS, and never into a TILES stream
inline bool lights_fit(const RenderArgs& r) {
  return r.l.n == 0 || (r.l.n > 0 && r.l.n <= SDF_MAX_LIGHTS && r.a.format != SDF_FORMAT_TILES &&
                        r.a.format != SDF_FORMAT_SHADE32F);
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
  return r.l.n > 0 && r.a.format != SDF_FORMAT_TILES && r.a.format != SDF_FORMAT_SHADE32F &&
         (prims ? r.m.n == r.a.prim_count && r.m.n > 0 : r.m.n == 0) && r.r.bounces >= 0 &&
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
// Shared by the built-in launchers (render_kernel.inc launch_rays_scene) and
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

}  // namespace sdf
