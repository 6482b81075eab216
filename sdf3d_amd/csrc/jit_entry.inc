// jit_entry.inc -- the entry point of a run-time specialised unit (jit.cpp).
// Included last by render_kernel.inc, inside namespace SDF_NS, when the unit
// defines SDF_JIT_SIGNATURE.  The entry is its family's kernel statement
// (SDF_*_KERNEL in the family's kernel file: launch bounds, occupancy and body,
// the very one the built-in kernels of the family are made from) for
// FixedScene<signature>, under an unmangled name.
//
// The contract -- what such a unit defines before it includes
// render_kernel.inc, and nothing else (jit.cpp jit_source writes these):
//   SDF_EXACT          0 | 1: the precision (render_kernel.inc)
//   SDF_JIT_SIGNATURE  FixedScene's argument list, the scene's (kind, op)
//                      codes separated by commas (kernel_args.h)
//   one family, by the macro that is defined:
//     SDF_JIT_RENDER   sdf_jit_render: render_body with SDF_JIT_TILES, _STEPS,
//                      _SSAA, _LIGHTS, _MATERIALS, _REFLECT, _ENV
//     SDF_JIT_QUERY    sdf_jit_query: query_body of the QueryKind it expands to
//     SDF_JIT_RAYS     sdf_jit_rays: rays_body with SDF_JIT_STEPS, SDF_JIT_ENV
//     SDF_JIT_MESH     sdf_jit_mesh: mesh_body of the MeshKind it expands to
//     SDF_JIT_POINTS   sdf_jit_points: points_body with SDF_JIT_STEPS
//     SDF_JIT_MEASURE  sdf_jit_measure: measure_body, with the owner rows when it
//                      expands to true
//   SDF_JIT_<flag>     true | false, each of the seven above (a family reads
//                      its own and ignores the rest)
// A signature is a primitive list, so the rays and points entries fold.

typedef FixedScene<SDF_JIT_SIGNATURE> JitScene;

#if defined(SDF_JIT_RENDER)
extern "C" SDF_RENDER_KERNEL(sdf_jit_render, JitScene, SDF_JIT_TILES, SDF_JIT_STEPS, SDF_JIT_SSAA,
                             SDF_JIT_LIGHTS, SDF_JIT_MATERIALS, SDF_JIT_REFLECT, SDF_JIT_ENV)
#elif defined(SDF_JIT_QUERY)
extern "C" SDF_QUERY_KERNEL(sdf_jit_query, JitScene, SDF_JIT_QUERY)
#elif defined(SDF_JIT_RAYS)
extern "C" SDF_RAYS_KERNEL(sdf_jit_rays, JitScene, SDF_JIT_STEPS, true, SDF_JIT_ENV)
#elif defined(SDF_JIT_MESH)
extern "C" SDF_MESH_KERNEL(sdf_jit_mesh, JitScene, SDF_JIT_MESH)
#elif defined(SDF_JIT_POINTS)
extern "C" SDF_POINTS_KERNEL(sdf_jit_points, JitScene, SDF_JIT_STEPS, true)
#elif defined(SDF_JIT_MEASURE)
extern "C" SDF_MEASURE_KERNEL(sdf_jit_measure, JitScene, SDF_JIT_MEASURE)
#else
#error "a run-time unit names its family: SDF_JIT_RENDER, _QUERY, _RAYS, _MESH, _POINTS or _MEASURE"
#endif
