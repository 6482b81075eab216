// render_launch.inc -- the host launchers of one render unit.
//
// Included behind render_kernel.inc by render_{exact,fast}.hip and
// render_{exact,fast}_bulb.hip; host code only: no kernel source (build.py
// KERNEL_SOURCES), so nothing of it is hashed or handed to hipRTC.
//
// Per kernel family one launch_*_scene<Scene>: the family's grid, its argument
// contract (host_api.h: the run-time specialised launchers of jit.cpp use the
// same functions) and the choice among the family's instantiations.  One
// with_scene maps a variant id to the Scene type for all of them.  The unit
// exports its launchers as one table (host_api.h RenderUnit): unit(), or
// bulb_unit() from the Mandelbulb's translation unit, in the precision's
// namespace.
//
// The kernels are emitted into the code object in the order in which the
// launchers below instantiate them; tools/asm_compare.py compares kernel by
// kernel and does not see that order.
#include <type_traits>

#include "host_api.h"

namespace sdf {

#ifdef SDF_STATS
extern "C" int sdf_debug_stats(unsigned long long* out, int n, int reset) {
  if (n > 128) n = 128;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(SDF_NS::g_sdf_stats), n * 8) != hipSuccess)
    return -1;
  if (reset) {
    static const unsigned long long zero[128] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(SDF_NS::g_sdf_stats), zero, sizeof(zero)) != hipSuccess)
      return -1;
  }
  return 0;
}
#endif

namespace SDF_NS {

// The Scene type of a variant id as a template argument: f(scene), with
// decltype(scene)::type the Scene.  A unit holds the kernels of its own scenes
// alone (build.py UNITS): the Mandelbulb's unit its one scene, the other unit
// every fixed variant and the generic scene.  The host sends a variant to the
// unit that has it (host_api.h render_unit); any other is refused.
template <class S>
struct SceneOf {
  using type = S;
};
template <class F>
static int with_scene(int variant, F&& f) {
#if SDF_TU_BULB
  if (variant != kVariantBulb) return (int)hipErrorInvalidValue;
  return f(SceneOf<BulbScene>{});
#else
  switch (variant) {
#define SDF_SCENE_CASE(id, ...) \
  case id:                      \
    return f(SceneOf<FixedScene<__VA_ARGS__>>{});
    SDF_FIXED_VARIANTS(SDF_SCENE_CASE)
#undef SDF_SCENE_CASE
    case kVariantBulb:
      return (int)hipErrorInvalidValue;
    default:
      return f(SceneOf<GenericScene>{});
  }
#endif
}

// The two run-time booleans of a launch -- step counts asked for, and a
// supersampled frame -- as template arguments: f(steps, ssaa), each a
// std::bool_constant.
template <class F>
static void with_steps_ssaa(const KernelArgs& a, F&& f) {
  using T = std::true_type;
  using N = std::false_type;
  if (a.ss_log2 > 0) a.steps ? f(T{}, T{}) : f(N{}, T{});
  else a.steps ? f(T{}, N{}) : f(N{}, N{});
}

// one launch of scene kernel S: its kernel family by the format and by what
// rides in the arguments (render_args_fit holds for them), and the
// step-recording instantiation only when the caller asked for step counts
template <class S, bool TILES>
static void launch_scene(const RenderArgs& a, dim3 grid, dim3 block, hipStream_t s) {
  constexpr bool kFold = !SDF_TU_BULB;   // a primitive list to fold materials over
#define SDF_GO(...) hipLaunchKernelGGL((SDF_NS::__VA_ARGS__), grid, block, 0, s, a)
  with_steps_ssaa(a.a, [&](auto steps, auto ssaa) {
    constexpr bool STEPS = decltype(steps)::value, SSAA = decltype(ssaa)::value;
    if constexpr (TILES) {
      SDF_GO(render_tiles<S, true, STEPS>);   // never supersampled (sdf_validate)
    } else if (a.e.on) {
      // a reflect launch with an environment (env_fit)
      SDF_GO(render_env<S, STEPS, SSAA, kFold>);
    } else if (a.r.on) {
      // mirror reflections (reflect_fit: lights, and a material table for every
      // scene with a primitive list; never TILES)
      SDF_GO(render_reflect<S, STEPS, SSAA, kFold>);
    } else if (a.m.n > 0) {
      // a material per primitive (materials_fit: never a Mandelbulb, which has
      // no primitive list to fold over; never TILES)
      if constexpr (kFold) SDF_GO(render_materials<S, STEPS, SSAA>);
    } else if (a.l.n > 0) {
      // several lights (the host refuses TILES with them)
      SDF_GO(render_lights<S, STEPS, SSAA>);
    } else if constexpr (SSAA) {
      SDF_GO(render_ssaa<S, STEPS>);
    } else {
      SDF_GO(render<S, false, STEPS>);
    }
  });
#undef SDF_GO
}

// the persistent frame-sequence kernel on `nblocks` 256-thread workgroups
template <class S>
static int launch_frames_scene(const FramesArgs& a, int nblocks, hipStream_t s) {
  if (a.nframes <= 0 || a.tiles_per_frame <= 0 || nblocks <= 0) return 0;
  bool steps = false;
  for (int i = 0; i < a.nframes; ++i) steps = steps || a.frame[i].steps != nullptr;
  (void)hipGetLastError();
  if (steps)
    hipLaunchKernelGGL((SDF_NS::render_frames<S, true>), dim3(nblocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((SDF_NS::render_frames<S, false>), dim3(nblocks), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

// one launch of scene kernel S for a query, on the family's grid and under
// its contract (host_api.h query_grid, query_args_fit)
template <class S>
static int launch_query_scene(const QueryArgs& q, hipStream_t s) {
  (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
  if (!query_args_fit(q)) return (int)hipErrorInvalidValue;
  const dim3 block(64 * kWgWaves), grid = query_grid(q);
  if (grid.x == 0 || grid.y == 0) return 0;
  if (q.kind == kQueryCamera)
    hipLaunchKernelGGL((SDF_NS::query<S, kQueryCamera>), grid, block, 0, s, q);
  else if (q.kind == kQueryRays)
    hipLaunchKernelGGL((SDF_NS::query<S, kQueryRays>), grid, block, 0, s, q);
  else
    hipLaunchKernelGGL((SDF_NS::query<S, kQueryPoints>), grid, block, 0, s, q);
  return (int)hipGetLastError();
}

static int launch_query(const QueryArgs& q, int variant, void* stream) {
  return with_scene(variant, [&](auto scene) {
    return launch_query_scene<typename decltype(scene)::type>(q, (hipStream_t)stream);
  });
}

// one launch of scene kernel S for a mesh extraction: one wave per brick,
// mesh_count, mesh_emit or mesh_emit_sharp (a MeshKind), under the family's
// contract (host_api.h mesh_args_fit, mesh_sharp_args_fit).  The Mandelbulb's
// unit has no sharp kernel: its scene has no analytic gradient.
template <class S>
static int launch_mesh_scene(const MeshArgs& m, int kind, hipStream_t s) {
  if (!mesh_args_fit(m)) return (int)hipErrorInvalidValue;
  const dim3 block(64), grid = mesh_grid(m);
  (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
  if (kind == kMeshEmitSharp) {
#if SDF_TU_BULB
    return (int)hipErrorInvalidValue;
#else
    if (!mesh_sharp_args_fit(m)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((SDF_NS::mesh_emit_sharp<S>), grid, block, 0, s, m);
#endif
  } else if (kind == kMeshEmit) {
    hipLaunchKernelGGL((SDF_NS::mesh_emit<S>), grid, block, 0, s, m);
  } else if (kind == kMeshCount) {
    hipLaunchKernelGGL((SDF_NS::mesh_count<S>), grid, block, 0, s, m);
  } else {
    return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

static int launch_mesh(const MeshArgs& m, int variant, void* stream, int kind) {
  return with_scene(variant, [&](auto scene) {
    return launch_mesh_scene<typename decltype(scene)::type>(m, kind, (hipStream_t)stream);
  });
}

// one launch of scene kernel S for sdf_measure: grid-stride, one wave per
// workgroup, under the family's contract (host_api.h measure_args_fit); the
// kernel with the owner rows when the arguments ask for them
template <class S>
static int launch_measure_scene(const MeasureArgs& m, hipStream_t s) {
  if (!measure_args_fit(m)) return (int)hipErrorInvalidValue;
  const dim3 block(64), grid = measure_grid(m);
  (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
  if (m.owners) hipLaunchKernelGGL((SDF_NS::measure<S, true>), grid, block, 0, s, m);
  else hipLaunchKernelGGL((SDF_NS::measure<S, false>), grid, block, 0, s, m);
  return (int)hipGetLastError();
}

static int launch_measure(const MeasureArgs& m, int variant, void* stream) {
  return with_scene(variant, [&](auto scene) {
    return launch_measure_scene<typename decltype(scene)::type>(m, (hipStream_t)stream);
  });
}

#if !SDF_TU_BULB
// sdf_sample_grad: the grid-stride gradient kernel, then the sum of its rows
// into `grad_prims` (device, kGradSlots floats) when it and g.rows are set.
// Primitive scenes only, always the generic unculled evaluator, whatever the
// variant.  The host (sdf_abi.cpp sdf_sample_grad) has bounded n and sized
// g.rows.
static int launch_grad(const GradArgs& g, int, void* stream, float* grad_prims) {
  if (g.n <= 0 || !g.points || (grad_prims != nullptr) != (g.rows != nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int nblocks = (int)grad_blocks(g.n);
  const dim3 block(kGradBlock), grid((unsigned)nblocks);
  (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
  if (grad_prims) {
    hipLaunchKernelGGL((SDF_NS::sample_grad<true>), grid, block, 0, s, g);
    hipLaunchKernelGGL(SDF_NS::grad_reduce, dim3(1), dim3(4 * kGradSlots), 0, s, g.rows, nblocks,
                       grad_prims);
  } else {
    hipLaunchKernelGGL((SDF_NS::sample_grad<false>), grid, block, 0, s, g);
  }
  return (int)hipGetLastError();
}
#endif

// one launch of scene kernel S for sdf_render_rays: 64 rays to a wave, the env
// kernels when an environment rides in the arguments, the step-recording
// instantiation only when the caller asked for step counts.  It refuses what
// the kernels' loops would trust blindly (host_api.h rays_args_fit).
template <class S>
static int launch_rays_scene(const RaysArgs& q, hipStream_t s) {
  constexpr bool kFold = !SDF_TU_BULB;   // a primitive list to fold materials over
  if (q.n <= 0) return 0;
  if (!rays_args_fit(q)) return (int)hipErrorInvalidValue;
  const dim3 block(64 * kWgWaves), grid(rays_grid(q));
  (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
#define SDF_GO(...) hipLaunchKernelGGL((SDF_NS::__VA_ARGS__), grid, block, 0, s, q)
  if (q.e.on) {
    if (q.a.steps) SDF_GO(render_rays_env<S, true, kFold>);
    else SDF_GO(render_rays_env<S, false, kFold>);
  } else {
    if (q.a.steps) SDF_GO(render_rays<S, true, kFold>);
    else SDF_GO(render_rays<S, false, kFold>);
  }
#undef SDF_GO
  return (int)hipGetLastError();
}

static int launch_rays(const RaysArgs& q, int variant, void* stream) {
  return with_scene(variant, [&](auto scene) {
    return launch_rays_scene<typename decltype(scene)::type>(q, (hipStream_t)stream);
  });
}

// one launch of scene kernel S for sdf_shade_points: 64 points to a wave, the
// instantiation whose shadow marches all run to the reference's break only
// when `shadow` or `steps` is asked for.  It refuses what the kernels would
// trust blindly (host_api.h points_args_fit).
template <class S>
static int launch_points_scene(const PointsArgs& q, hipStream_t s) {
  constexpr bool kFold = !SDF_TU_BULB;   // a primitive list to fold materials over
  if (q.n <= 0) return 0;
  if (!points_args_fit(q)) return (int)hipErrorInvalidValue;
  const dim3 block(64 * kWgWaves), grid(points_grid(q));
  (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
  if (points_steps(q))
    hipLaunchKernelGGL((SDF_NS::shade_points<S, true, kFold>), grid, block, 0, s, q);
  else
    hipLaunchKernelGGL((SDF_NS::shade_points<S, false, kFold>), grid, block, 0, s, q);
  return (int)hipGetLastError();
}

static int launch_points(const PointsArgs& q, int variant, void* stream) {
  return with_scene(variant, [&](auto scene) {
    return launch_points_scene<typename decltype(scene)::type>(q, (hipStream_t)stream);
  });
}

#if !SDF_TU_BULB
// sdf_camera_rays: the render's grid of 8x8 tiles over width x height; one
// kernel, whatever the variant
static int launch_camera_rays(const RaysArgs& q, int, void* stream) {
  const dim3 block = render_block();
  const dim3 grid((q.a.width + 8 * kWgWaves - 1) / (8 * kWgWaves), (q.a.height + 7) / 8);
  if (q.a.width <= 0 || q.a.height <= 0 || (!q.out0 && !q.out1)) return (int)hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(SDF_NS::camera_rays, grid, block, 0, (hipStream_t)stream, q);
  return (int)hipGetLastError();
}
#endif

// one render on the render grid, under the render's contract (host_api.h
// render_grid, render_args_fit): the TILES kernels or the others, of the
// variant's scene
static int launch_render(const RenderArgs& a, int variant, void* stream) {
  const dim3 block = render_block(), grid = render_grid(a.a);
  if (grid.x == 0 || grid.y == 0) return 0;
  if (!render_args_fit(a, grid)) return (int)hipErrorInvalidValue;
  const auto launch = [&](auto tiles) {
    return with_scene(variant, [&](auto scene) {
      (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
      launch_scene<typename decltype(scene)::type, decltype(tiles)::value>(a, grid, block,
                                                                           (hipStream_t)stream);
      return (int)hipGetLastError();
    });
  };
  return a.a.format == SDF_FORMAT_TILES ? launch(std::true_type{}) : launch(std::false_type{});
}

static int launch_frames(const FramesArgs& a, int variant, void* stream, int nblocks) {
  return with_scene(variant, [&](auto scene) {
    return launch_frames_scene<typename decltype(scene)::type>(a, nblocks, (hipStream_t)stream);
  });
}

// The unit's table.  No ray generator and no gradient kernel in the Mandelbulb's:
// neither depends on the scene.
#if SDF_TU_BULB
const RenderUnit& bulb_unit() {
  static const RenderUnit u = {launch_render, launch_frames, launch_query, launch_rays,
                               launch_mesh,   launch_points, launch_measure, nullptr,
                               nullptr};
  return u;
}
#else
const RenderUnit& unit() {
  static const RenderUnit u = {launch_render, launch_frames, launch_query,       launch_rays,
                               launch_mesh,   launch_points, launch_measure,
                               launch_camera_rays, launch_grad};
  return u;
}
#endif

}  // namespace SDF_NS
}  // namespace sdf
