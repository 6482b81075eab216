// render_kernel.inc -- the per-pixel SDF sphere-tracing kernel for gfx950.
//
// Included by render_exact.hip (SDF_EXACT = 1, compiled -ffp-contract=off with
// IEEE div/sqrt: the same fp32 operation sequence as the fragment shader, so
// the output is bit-comparable with the CPU oracle) and by render_fast.hip
// (SDF_EXACT = 0: FMA contraction, v_sqrt/v_rcp/v_rsq, min/max instructions).
//
// What one lane computes = fragment-stage main() of the reference,
// /root/reference/Code/shader/voxel_fragment.frag:160-211, for one pixel:
//   ray generation (:191-192, pixel -> quad from voxel_geometry.geom:26-52)
//   raymarch (:86-103) -> normal (:134-155, or tetrahedral) -> Blinn-Phong
//   (:200-204) -> soft shadow (:105-132, :205) -> [AO] -> colour (:206-210).
//
// Mapping: one lane = one pixel; one wave64 = an 8x8 pixel tile (rays of a
// tile are coherent, so the march loop's exec mask stays full longer and the
// wave leaves the loop as soon as its last lane converges); a workgroup is
// kWgWaves tiles side by side (kernel_args.h: one).  Scene constants come from
// the kernel-argument segment with scalar loads.  The only HBM traffic is the
// 16-byte float4 store per pixel (row-contiguous 128-byte segments per tile row).
//
// Device code only: the four render units include their host launchers
// behind this file (render_launch.inc); hipRTC compiles this file alone.
//
// This file holds the configuration and the order of the layers; the code is
// in the layer files included below (build.py KERNEL_SOURCES lists them all).

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <math.h>
#else
// compiled at run time by hipRTC for one scene signature (jit.cpp)
#define INFINITY __builtin_inff()
#endif

#include "kernel_args.h"
#include "wave_bits.h"
#include "shade.h"
#if SDF_EXACT
// cr_math.h's one-compare square-root guard (cr_sqrt exact for every finite
// argument) in the CSG units: there sdf_validate's working range (every
// coordinate, size and distance <= 1e15) keeps every squared length below
// ~1e33, so +INF never reaches it.  The Mandelbulb unit's orbit may overflow:
// the full range test (every x).
#if !defined(SDF_CRM_SQRT_GUARD) && !defined(SDF_TU_BULB)
#define SDF_CRM_SQRT_GUARD 1
#endif
#include "cr_math.h"
#endif

#ifndef SDF_EXACT
#error "SDF_EXACT must be 0 or 1"
#endif

// Waves per SIMD the render kernels are built for (the VGPR budget): 8 =
// 64 VGPRs.  Overridable per build for occupancy experiments.
#ifndef SDF_WAVES_PER_EU
#define SDF_WAVES_PER_EU 8
#endif
// What every kernel entry begins with: the workgroup size it is launched with
// and the waves per SIMD it is built for (minimum = maximum).
#define SDF_KERNEL(threads, waves) \
  __global__ __launch_bounds__(threads) __attribute__((amdgpu_waves_per_eu(waves, waves)))
// The workgroup bound of the entries launched with 64 kWgWaves lanes (render,
// query, rays, points): that size in the built-in units.  A run-time unit has
// always been built for 256, and the bound enters the instruction stream (the
// same kernel at 64 differs in a few instructions), so it stays until a pull
// request of its own measures the two.
#ifdef SDF_JIT_SIGNATURE
#define SDF_WG_BOUND 256
#else
#define SDF_WG_BOUND (64 * kWgWaves)
#endif

// Stage ablation (tools/ablate.py): 1 skips the normal's taps, so a frame's
// time splits into primary march, normal, AO and shadow.  Experiment builds
// only (tools/flag_variant.py defines SDF_EXPERIMENT).
#ifndef SDF_ABLATE_NO_NORMAL
#define SDF_ABLATE_NO_NORMAL 0
#endif
#if SDF_ABLATE_NO_NORMAL && !defined(SDF_EXPERIMENT)
#error "SDF_ABLATE_NO_NORMAL renders wrong pixels: experiment builds only"
#endif

// SDF_TU_BULB 1: this translation unit holds the Mandelbulb scene's kernels
// alone (render_{fast,exact}_bulb.hip), built with a scheduler of its own
// (build.py); 0: every other scene.
#ifndef SDF_TU_BULB
#define SDF_TU_BULB 0
#endif
#if SDF_EXACT
#define SDF_NS exact_impl
#else
#define SDF_NS fast_impl
#endif

namespace sdf {
namespace SDF_NS {

// The layers, each a file of its own included here and nowhere else (no
// guards, none includes another): a file uses what the ones above it define.
#include "kmath.inc"            // KARG / KA / KF, V3, Seq, the precision's arithmetic
#include "prims.inc"            // sd_*, smin, combine, the folds' steps, the Mandelbulb map, sel_*
#include "store.inc"            // store_pixel, the TILES encoder
#include "scenes.inc"           // MarchState, culling, taps, GenericScene, FixedScene, BulbScene
#include "trace.inc"            // the views, Surface, trace_*, light_terms
#include "pixel_paths.inc"      // shade_pixel*, surface_colour, ReflectPath, env_layer
#include "render_entry.inc"     // the resolve, render_body, the render kernels, render_frames
#include "query_kernel.inc"     // sdf_trace, sdf_trace_camera, sdf_sample
#if !SDF_TU_BULB
#include "grad_kernel.inc"      // sdf_sample_grad
#endif
#include "mesh_kernel.inc"      // sdf_mesh_count, sdf_mesh_emit, sdf_mesh_emit_sharp
#include "measure_kernel.inc"   // sdf_measure
#include "rays_kernel.inc"      // sdf_render_rays, sdf_camera_rays
#include "points_kernel.inc"    // sdf_shade_points
#ifdef SDF_JIT_SIGNATURE
#include "jit_entry.inc"        // a run-time unit's extern "C" entry (the contract is there)
#endif

#undef SDF_KERNEL
#undef SDF_WG_BOUND
#undef SDF_RENDER_KERNEL
#undef SDF_QUERY_KERNEL
#undef SDF_MESH_KERNEL
#undef SDF_MEASURE_KERNEL
#undef SDF_RAYS_KERNEL
#undef SDF_POINTS_KERNEL
#undef scene_sdf
#undef DIVK
#undef SMIN_K
#undef SMIN_IK
#undef SMIN_SC
#undef SMIN_KSC

}  // namespace SDF_NS

}  // namespace sdf
