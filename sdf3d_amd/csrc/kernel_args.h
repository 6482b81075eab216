// kernel_args.h -- uniform block handed from the C-ABI host code to the HIP
// render kernels.  Everything here is per-frame constant: the host hoists the
// shader's uniform-only work (inverse(V_mat) twice per pixel, camera.pos, the
// focal term -2/tan(fov*PI/360); voxel_fragment.frag:180, :191-192) so each
// lane only does per-pixel arithmetic.  Passed by value as the kernel argument
// so the fields are read with scalar loads (SGPRs), never per lane.
//
// Kernel source: hipRTC compiles it with render_kernel.inc, and it enters
// sdf_kernel_id.  Argument blocks, buffer layouts and the constants kernels
// and host share live here; every host function's prototype in host_api.h.
#pragma once

#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdint.h>
#else
typedef __hip_internal::uint8_t uint8_t;
typedef __hip_internal::uint16_t uint16_t;
typedef __hip_internal::uint32_t uint32_t;
typedef __hip_internal::uint64_t uint64_t;
#endif

#include "../../include/sdf_abi.h"

namespace sdf {

constexpr int kMaxAoTaps = 64;

struct KernelArgs {
  // camera (hoisted uniforms)
  float inv_view[16];   // inverse(V_mat), column-major
  float cam[3];         // (inverse(V_mat) * vec4(camera.pos, 1)).xyz
  float focal;          // -2 / tan(fov * PI / 360)
  float aspect;         // AR
  // light + material (voxel_fragment.frag:182-189)
  float light_pos[3];
  float light_amb;
  float mat_amb[3];
  float mat_dif[3];
  float mat_ref[3];
  float shininess;
  // march parameters
  int32_t width, height;
  int32_t max_steps;
  float max_dist, eps, shadow_k, normal_eps, shadow_offset;
  int32_t flags, normal_mode, format;
  int32_t ao_taps;
  float ao_step, ao_base, ao_falloff, ao_strength;
  float ao_h[kMaxAoTaps];  // tap heights base + step * i / (taps - 1), host fp32
  float ao_path[kMaxAoTaps];  // path length P -> tap 0 -> .. -> tap i (fp64, rounded up)
  float inv_width, inv_height;  // fast precision quad mapping
  // tiling
  int32_t block_rows, first_block, block_stride, rows;
  int32_t chunk_rows;   // block_rows * run: rows of one period's run of blocks
  int32_t run_gap_rows; // (run_step - 1) * block_rows: rows skipped between a run's blocks
  int32_t frame_rows;   // SDF_TILING_FRAME_ROWS: output row = frame row y
  // scene
  int32_t scene_kind, prim_count;
  float bulb_center[3], bulb_scale, bulb_inv_scale, bulb_bail2;
  int32_t bulb_iterations;
  // prepared primitives (sdf_abi.cpp prepare_prims): kind, op, k,
  // reserved = 1/k, p = per-kind parameter block (see prims.inc)
  sdf_primitive prims[SDF_MAX_PRIMS];
  // culling bounds (fixed-scene kernels): per primitive {centre.xyz, K} with
  // K = k + R + margin, R the radius of a sphere containing the primitive;
  // and the same for the cluster of primitives [cluster_first, count)
  alignas(16) float bound[SDF_MAX_PRIMS][4];   // 16-B aligned: read as float4 vector loads
  alignas(16) float cluster[4];
  int32_t cluster_first;
  // outputs
  void* rgba;           // rows * width pixels of `format`, packed rows
  int32_t* steps;       // rows * width int2 or null
  // supersampling (sdf_params.samples = S > 1, render_ssaa): width, height,
  // rows and the tiling above are then those of the S W x S H sub-sample
  // frame, `steps` its buffer, and `rgba` holds rows / S rows of out_width =
  // width / S resolved pixels
  int32_t out_width;    // pixels per output row (width when S = 1)
  int32_t ss_log2;      // log2 S: 0 (one sample per pixel), 1 or 2
};

// ---- dispatch order of a frame's 8-row blocks (sdf_render_scheduled) -------
// The render grid's row of workgroups blockIdx.y renders packed 8-row block
// order[blockIdx.y] (n > 0; launch order otherwise): a schedule puts the
// blocks that cost most in earlier frames first, so the frame's longest tiles
// do not run alone at its end.  The table rides in the kernel-argument
// segment (never a buffer another frame may be rewriting): any permutation
// renders every block exactly once.  `cost` (may be null): each wave adds the
// shader-clock cycles it took to its block's word.
constexpr int kMaxOrderBlocks = 512;   // 4096 packed rows
struct RowOrder {
  unsigned long long* cost;
  int32_t n;
  int32_t reserved;
  uint16_t order[kMaxOrderBlocks];
};
// ---- several lights (sdf_render_lights) ------------------------------------
// The lights of a multi-light render ride in the kernel-argument segment
// behind the row order, so the kernel's loop over them reads scalars: light
// i's position and colour, the summed ambient `la` (fp32, index order) and
// the SDF_LIGHTS_* flags.  n = 0: a plain render, which reads none of this
// (KernelArgs::light_pos / light_amb are the one light's).
struct LightsArgs {
  float pos[SDF_MAX_LIGHTS][3];
  float color[SDF_MAX_LIGHTS][3];
  float la;
  int32_t n;
  int32_t flags;
  int32_t reserved;
};
// ---- per-primitive materials (sdf_render_materials) ------------------------
// m[i] = primitive i's material as 9 components (amb, dif, ref), read with
// scalar loads by the material fold at P (scenes.inc material_fold).
// The shininess stays KernelArgs::shininess (frame-wide).  n = 0: one material
// for the frame (KernelArgs::mat_*), nothing here is read.
struct MaterialArgs {
  float m[SDF_MAX_PRIMS][9];
  int32_t n;
  int32_t reserved[3];
};
// ---- mirror reflections (sdf_render_reflect) --------------------------------
// The uniforms of the loop over a pixel's layers (pixel_paths.inc
// shade_pixel_reflect): sdf_reflect's fields as the host validated them.
// on = 0: no reflect kernel, nothing here is read.
struct ReflectArgs {
  int32_t on;
  int32_t bounces;
  float strength;
  int32_t layer;    // -1 the composite, else the one layer written
  int32_t weight;   // SDF_REFLECT_WEIGHT: write W_layer instead of C_layer
  int32_t reserved[3];
};
// ---- environment (sdf_render_env) -------------------------------------------
// The uniforms of a missed layer's sky and of the distance fog (pixel_paths.inc
// shade_pixel_env, shade.h env_sky / env_fog): sdf_environment's fields as the
// host validated them, with the fog's denominator RN(fog_end - fog_start)
// (exact precision divides by it) and its reciprocal RN(1 / den) (fast
// precision multiplies).  Fields of a feature whose flag is off are zero and
// never read.  on = 0: no env kernel, nothing here is read.
struct EnvArgs {
  int32_t on;
  int32_t flags;        // SDF_ENV_*
  float horizon[3], zenith[3], ground[3];
  float sun_dir[3], sun_color[3], sun_exponent;
  float fog_color[3], fog_end, fog_den, fog_inv;
};
struct RenderArgs {
  KernelArgs a;   // first: the kernels read it at the start of the segment
  RowOrder o;
  LightsArgs l;   // only RenderArgs has the room (FramesArgs is near 4 KiB)
  MaterialArgs m; // behind the lights: a materials render always has lights (l.n >= 1)
  ReflectArgs r;  // behind the materials: a reflect render has lights, and a table per primitive
  EnvArgs e;      // behind the reflect block: an env render is a reflect render (bounces >= 0)
};
// ---- queries (sdf_trace, sdf_trace_camera, sdf_sample) ------------------------
// The argument block of the query kernels (query_kernel.inc query_rays /
// query_camera / query_points), their own: RenderArgs is full (4096 bytes).
// `a` carries the scene, the march parameters and, for camera rays, the
// hoisted camera and the frame size; its outputs (rgba, steps) are unused.
// `in0` holds n x 3 packed floats (ray origins, or the points of a sample),
// `in1` the ray directions.  Which outputs are written is a uniform branch on
// their pointers (any may be null, not all).
enum QueryKind : int32_t { kQueryRays = 0, kQueryCamera = 1, kQueryPoints = 2 };
struct QueryArgs {
  KernelArgs a;   // first: the scene evaluators read it at the start of the segment
  const float* in0;
  const float* in1;
  float* t;         // n: the march's distance (points: the scene distance)
  int32_t* steps;   // n: the march's iteration count
  float* normal;    // 3 n, packed xyz
  int32_t* prim;    // n: the owner fold's primitive, -1 on a miss
  long long n;      // rays or points (camera rays: width * height)
  int32_t kind;     // QueryKind
  int32_t reserved;
};
// ---- caller-supplied rays (sdf_render_rays, sdf_camera_rays) -------------------
// The argument block of the rays kernels (rays_kernel.inc render_rays /
// render_rays_env / camera_rays), their own: RenderArgs is full, and its
// RowOrder is of no use to a list of rays.  `a` carries the scene, the march
// and shading parameters and the outputs (a.rgba: n pixels of a.format,
// a.steps: n int2 or null; camera_rays: the hoisted camera and the frame
// size); l, m, r and e are a render's.  `in0` holds n x 3 packed floats (ray
// origins), `in1` the directions; camera_rays writes through `out0` / `out1`
// (either may be null).
struct RaysArgs {
  KernelArgs a;   // first: the scene evaluators read it at the start of the segment
  LightsArgs l;
  MaterialArgs m;
  ReflectArgs r;  // on = 1 always: no bounce is bounces 0 with layer -1
  EnvArgs e;      // on = 0: the reflect layers (render_rays), else render_rays_env
  const float* in0;
  const float* in1;
  float* out0;
  float* out1;
  long long n;    // rays
  int32_t flags;  // SDF_RAYS_*
  int32_t reserved;
};
// ---- shading at caller-supplied points (sdf_shade_points) ----------------------
// The argument block of the points kernels (points_kernel.inc shade_points),
// their own: `a` carries the scene, the march and shading parameters (its camera,
// frame size and outputs are unused; a.ao_taps is 0 when no output needs the
// occlusion term); l and m are a materials render's.  `points` holds n x 3
// packed floats, `normals` the same or null (the normal's taps run at the
// point).  Which outputs are written is a uniform branch on their pointers
// (any may be null, not all): rgba n x 4, ao n, shadow and steps n x l.n,
// material n x 9.
struct PointsArgs {
  KernelArgs a;   // first: the scene evaluators read it at the start of the segment
  LightsArgs l;
  MaterialArgs m;   // n = 0: a Mandelbulb, the one material of `a`
  const float* points;
  const float* normals;
  float* rgba;
  float* ao;
  float* shadow;
  float* material;
  int32_t* steps;
  long long n;    // points
  float eye[3];   // with SDF_POINTS_EYE
  float lift;
  int32_t flags;  // SDF_POINTS_*
  int32_t reserved;
};
// ---- isosurface meshes (sdf_mesh_count, sdf_mesh_emit) -------------------------
// The workspace of a mesh extraction (sdf_abi.h "Meshes"), O(bricks): per
// brick of 8 x 8 x 8 cells its 512-bit activity mask (word l2: the 8 x 8 slice
// l2, bit l1 * 8 + l0), two counts and two offsets, then the scan's
// per-chunk sums.  sdf_mesh_workspace_bytes() = end.
constexpr int kMeshScanChunk = 1024;          // bricks per workgroup of the offset scan
constexpr uint32_t kMeshEvaluated = 1u << 31; // MeshBrick::nv: the brick's lattice was evaluated
struct MeshBrick {
  uint32_t nv;   // vertices (active cells), <= 512; | kMeshEvaluated
  uint32_t nt;   // triangles, <= 3072
};
struct MeshOffset {
  long long v, t;   // vertices / triangles of the bricks before this one
};
struct MeshLayout {
  size_t mask, brick, offset, sums, end;
  __host__ __device__ explicit MeshLayout(long long nbricks) {
    const size_t n = (size_t)nbricks;
    const size_t chunks = (n + kMeshScanChunk - 1) / kMeshScanChunk;
    mask = 0;
    brick = mask + 64 * n;
    offset = brick + sizeof(MeshBrick) * n;
    sums = offset + sizeof(MeshOffset) * n;
    end = sums + 3 * sizeof(long long) * chunks;
  }
};
// The argument block of the mesh kernels (mesh_kernel.inc mesh_count /
// mesh_emit / mesh_emit_sharp), their own: RenderArgs is full.  `a` carries the scene and the
// normal's parameters; its camera, light and outputs are unused.
struct MeshArgs {
  KernelArgs a;   // first: the scene evaluators read it at the start of the segment
  float origin[3], cell[3];
  int32_t n[3];        // cells per axis
  int32_t nb[3];       // bricks per axis, ceil(n / 8)
  float iso;
  float skip;          // a brick is skipped when |f(centre) - iso| > skip (+INF: never)
  long long nbricks;
  unsigned char* ws;   // MeshLayout(nbricks)
  float* verts;        // emit: 3 per vertex, vertex v stored iff v < max_verts
  int32_t* tris;       // emit: 3 per triangle, triangle t stored iff t < max_tris
  float* normal;       // emit, optional: 3 per vertex
  int32_t* prim;       // emit, optional: 1 per vertex
  long long max_verts, max_tris;
  int32_t refine;      // mesh_emit_sharp: regula-falsi steps per crossing edge, 0 .. 8
  int32_t iterations;  // mesh_emit_sharp: descent steps of the vertex fit, 0 .. 64
};
// the kernel of a mesh launch (RenderUnit::mesh, launch_mesh_jit: `kind`)
enum MeshKind { kMeshCount = 0, kMeshEmit = 1, kMeshEmitSharp = 2 };
// ---- measures (sdf_measure) ------------------------------------------------------
// The argument block of the measure kernels (measure_kernel.inc measure), their
// own: `a` carries the prepared scene, nothing else of it is read.  A
// grid-stride launch of at most kMeasureMaxBlocks one-wave workgroups over the
// mesh's bricks; each workgroup writes one record to `ws`, the workspace: its
// rows (1, or SDF_MEASURE_ROWS with owners) of SDF_MEASURE_SLOTS int64, then
// kMeasureTail int64 (bricks evaluated, bricks in closed form, 0, 0), which
// measure_reduce (mesh.hip) combines: sums, and min / max for lo / hi.
// sdf_measure_workspace_bytes() = 8 measure_blocks(nbricks) measure_record(rows).
constexpr int kMeasureMaxBlocks = 4096;   // 4 waves per SIMD of 256 CUs
constexpr int kMeasureTail = 4;
// slots [0, kMeasureSums) of a row are sums, the next three minima, the last three maxima
constexpr int kMeasureSums = 10;
constexpr int kMeasureLo = 10, kMeasureHi = 13;
__host__ __device__ inline long long measure_blocks(long long nbricks) {
  return nbricks < kMeasureMaxBlocks ? nbricks : kMeasureMaxBlocks;
}
__host__ __device__ constexpr int measure_rows(bool owners) { return owners ? SDF_MEASURE_ROWS : 1; }
__host__ __device__ constexpr int measure_record(int rows) {
  return rows * SDF_MEASURE_SLOTS + kMeasureTail;
}
struct MeasureArgs {
  KernelArgs a;   // first: the scene evaluators read it at the start of the segment
  float origin[3], cell[3];
  int32_t n[3];        // cells (samples) per axis, <= 65536
  int32_t nb[3];       // bricks per axis, ceil(n / 8)
  float iso;
  float skip;          // MeshArgs::skip, the same bound (+INF: every brick is evaluated)
  long long nbricks;
  long long* ws;       // measure_blocks(nbricks) records
  int32_t owners;      // SDF_MEASURE_OWNERS: the launch is of the kernel with the owner rows
  int32_t reserved;
};
// ---- gradients (sdf_sample_grad) ------------------------------------------------
// The argument block of the gradient kernel (grad_kernel.inc sample_grad), its
// own: `a` carries the prepared scene, nothing else of it is read.  A grid-stride
// launch of at most kGradMaxBlocks workgroups of kGradBlock lanes; with
// grad_prims each workgroup writes one row of kGradSlots floats (the layout of
// grad_prims) to `rows`, the workspace, which grad_reduce sums.
constexpr int kGradBlock = 256;                  // threads per workgroup (4 waves)
constexpr int kGradMaxBlocks = 1024;
constexpr int kGradSlots = 16 * SDF_MAX_PRIMS;   // floats of grad_prims and of a workspace row
struct GradArgs {
  KernelArgs a;   // first: the scene evaluators read it at the start of the segment
  const float* points;
  const float* upstream;   // n, or null: every g_i = 1
  float* dist;             // n, optional
  float* grad_points;      // 3 n, optional
  float* rows;             // grad_blocks(n) rows of kGradSlots floats, or null (no grad_prims)
  long long n;
};
__host__ __device__ inline long long grad_blocks(long long n) {
  const long long b = (n + kGradBlock - 1) / kGradBlock;
  return b < kGradMaxBlocks ? b : kGradMaxBlocks;
}

// Waves (8x8 tiles side by side) per render workgroup (render_entry.inc
// render / render_tiles / render_ssaa; the built-in and the run-time
// specialised launchers).
// Round 4: one wave per workgroup -- each wave is placed on its own, so the
// frame's last, longest tiles pack onto the CUs better than in 4-wave groups
// that need four slots of one CU: C4 fast 0-1.6 % faster, C5 fast up to 4 %,
// C4/C5 exact 0.2-1.8 % (profiles/r04_ab_workgroup.json; 2 waves lie between,
// 8 are 3-5 % slower).  Overridable for experiments (SDF_WG_WAVES).
#ifndef SDF_WG_WAVES
#define SDF_WG_WAVES 1
#endif
constexpr int kWgWaves = SDF_WG_WAVES;

// ---- frame sequences (sdf_render_frames) ----------------------------------
// Up to kFramesPerLaunch whole frames of one scene in one launch of a
// persistent kernel: its waves take 8x8 tiles of all the launch's frames from
// one work counter, frame after frame, so a frame's slowest tiles overlap the
// next frame's first ones instead of ending a launch.  The per-frame uniforms
// ride in the kernel-argument segment beside the shared KernelArgs (whose own
// camera and output fields are unused): sizeof(KernelArgs) + 16 x 104 bytes,
// checked below against the 4 KiB explicit kernel-argument limit.
constexpr int kFramesPerLaunch = 16;
struct FrameCam {
  float inv_view[16];   // inverse(V_mat) of this frame's camera
  float cam[3];
  float focal, aspect;
  void* rgba;           // width * height pixels of the params' format
  int32_t* steps;       // width * height int2 or null
};
struct FramesArgs {
  KernelArgs a;
  FrameCam frame[kFramesPerLaunch];
  int32_t nframes;          // 1 .. kFramesPerLaunch
  int32_t tiles_x;          // ceil(width / 8)
  int32_t tiles_per_frame;  // tiles_x * ceil(height / 8)
  int32_t queues;           // work queues (1 .. kFrameQueues, <= workgroups)
  int32_t schedule;         // 0 work queues, 1 static (tools/frames_probe.py)
  int32_t chunk;            // tiles per queue request (kChunkTiles)
  uint32_t* counter;        // queue q's counter at counter[q * kQueueStride], zero at launch
};
// the by-value kernel argument must fit the 4 KiB kernarg limit:
// raising kMaxAoTaps, SDF_MAX_PRIMS or kFramesPerLaunch fails here, not at launch
static_assert(sizeof(FramesArgs) <= 4096, "FramesArgs exceeds the 4 KiB kernel-argument limit");
static_assert(sizeof(KernelArgs) <= 4096, "KernelArgs exceeds the 4 KiB kernel-argument limit");
static_assert(sizeof(RenderArgs) <= 4096, "RenderArgs exceeds the 4 KiB kernel-argument limit");
static_assert(sizeof(QueryArgs) <= 4096, "QueryArgs exceeds the 4 KiB kernel-argument limit");
static_assert(sizeof(RaysArgs) <= 4096, "RaysArgs exceeds the 4 KiB kernel-argument limit");
static_assert(sizeof(PointsArgs) <= 4096, "PointsArgs exceeds the 4 KiB kernel-argument limit");
static_assert(sizeof(MeshArgs) <= 4096, "MeshArgs exceeds the 4 KiB kernel-argument limit");
static_assert(sizeof(GradArgs) <= 4096, "GradArgs exceeds the 4 KiB kernel-argument limit");
static_assert(sizeof(MeasureArgs) <= 4096, "MeasureArgs exceeds the 4 KiB kernel-argument limit");
// Tiles a wave takes per queue request, queues per launch (workgroup b uses
// queue b % queues, i.e. one per XCD), and the queues' spacing in uint32s:
// requests on one address serialise at the memory-side atomic unit, so the
// launch spreads them over several addresses.  One tile per request since
// round 6: the same rate on 16-frame launches (r02 sweep: 0.3665 against
// 0.3663 ms per frame with 2), and a ONE-frame launch 0.384 -> 0.237 ms on
// C3 exact, where larger requests leave waves without tiles (a 1080p frame
// has ~4 tiles per wave; profiles/r06_frames1_env.jsonl).
constexpr int kChunkTiles = 1;
constexpr int kFrameQueues = 32;   // at most; kDefaultQueues by default
constexpr int kDefaultQueues = 8;
constexpr int kQueueStride = 64;

// TILES decode of parts with their own tilings (sdf_tiles_decode_tilings)
struct DecodeParts {
  int nparts, width, height;
  long long part_stride;
  int rows[SDF_MAX_DECODE_PARTS], first_block[SDF_MAX_DECODE_PARTS],
      block_stride[SDF_MAX_DECODE_PARTS], block_rows[SDF_MAX_DECODE_PARTS],
      chunk_rows[SDF_MAX_DECODE_PARTS], run_gap_rows[SDF_MAX_DECODE_PARTS];
  // part r's stream at part_ptr[r] when non-null (another device's memory,
  // peer-mapped: sdf_render_multi), else at parts + r * part_stride
  const void* part_ptr[SDF_MAX_DECODE_PARTS];
  // A stream is untrusted input (it crossed RCCL): the decoder reads nothing
  // outside the part's worst-case stream.  used[r] >= 0: the data bytes part
  // r must hold (the length the ranks agreed on; its header word 0 must say
  // the same); -1: the header's word 0, at most the part's capacity.
  long long used[SDF_MAX_DECODE_PARTS];
  // device-writable, nparts words (may be null): word r is set to a nonzero
  // kTilesBad* code when part r is malformed (the decoder then skips the
  // part, or the tiles that are out of bounds, and writes nothing for them)
  uint32_t* status;
  // everything zero, no expected lengths (used = -1), no status words
  __host__ DecodeParts() {
    __builtin_memset(this, 0, sizeof(*this));
    for (int r = 0; r < SDF_MAX_DECODE_PARTS; ++r) used[r] = -1;
  }
};
// (sdf_abi.h SDF_TILES_BAD_*)
constexpr uint32_t kTilesBadHeader = SDF_TILES_BAD_HEADER;   // length / tile count disagree
constexpr uint32_t kTilesBadTile = SDF_TILES_BAD_TILE;       // a tile's offset, size or widths
constexpr uint32_t kTilesBadField = SDF_TILES_BAD_FIELD;     // an escape field past its tile

// ---- TILES stream buffer (sdf_abi.h SDF_FORMAT_TILES) ----------------------
// The buffer handed to sdf_render holds the stream (header, offset table,
// per-tile heads, worst-case plane data) followed by the encoder's scratch:
// per-block plane-byte totals of the offset scan and fixed worst-case plane
// slots.  sdf_tiles_bytes() = end.
constexpr int kTilePlaneBytes = 8 * 96;   // 3 channels x 32 planes
constexpr int kScanTiles = 2048;          // tiles per block of the offset scan
constexpr int kTilesHeaderBytes = 64;     // used, ntiles, shade mode, 0, ShadeK, 0, 0
struct TilesLayout {
  size_t table, head, data, stream_end, bsums, slots, end;
  __host__ __device__ explicit TilesLayout(long long ntiles) {
    const size_t n = (size_t)ntiles;
    const size_t nb = (n + kScanTiles - 1) / kScanTiles;
    table = kTilesHeaderBytes;
    head = (kTilesHeaderBytes + 4 * n + 15) & ~(size_t)15;
    data = head + 16 * n;
    stream_end = data + n * kTilePlaneBytes;
    bsums = (stream_end + 15) & ~(size_t)15;
    slots = (bsums + 4 * nb + 15) & ~(size_t)15;
    end = slots + n * kTilePlaneBytes;
  }
};
// A tile's head word 0 (sdf_abi.h SDF_FORMAT_TILES): base widths b0 | b1 << 6
// | b2 << 12, the tile's data in qwords << 18, escaped channels << 26.
__host__ __device__ inline uint32_t tile_qwords(uint32_t head) { return (head >> 18) & 255u; }
constexpr int kEscapeWindow = 12;   // base widths tried below the widest residual
constexpr int kEscapeDwords = 72;   // bitstream bound: 3 width bytes + 3 x 12 x 63 bits

// ---- compile-time scene variants ------------------------------------------
// A variant fixes the (kind, op) sequence of the primitive list at compile
// time; parameter values stay runtime uniforms.  The host picks the variant
// whose signature equals the scene's (host_api.h select_variant); anything
// else runs the generic kernel, which reads kinds and ops at run time.

// Internal primitive kind: a PLANE whose normal is exactly (0,1,0), evaluated
// as p.y + h -- the reference's planeSDF (voxel_fragment.frag:68) when h = 0.
constexpr int kPrimPlaneY = 7;
#define SDF_KO(kind, op) ((kind) * 8 + (op))

// X(variant id, signature...)
#define SDF_FIXED_VARIANTS(X)                                                        \
  /* reference scene: min(min(INF, plane), sphere), voxel_fragment.frag:73-81 */   \
  X(1, SDF_KO(kPrimPlaneY, SDF_OP_UNION), SDF_KO(SDF_PRIM_SPHERE, SDF_OP_UNION))    \
  /* C1: single sphere */                                                          \
  X(2, SDF_KO(SDF_PRIM_SPHERE, SDF_OP_UNION))                                      \
  /* C3/C4: 8-primitive smooth-min CSG (sdf3d_amd/scenes.py set_csg8) */           \
  X(3, SDF_KO(kPrimPlaneY, SDF_OP_UNION), SDF_KO(SDF_PRIM_SPHERE, SDF_OP_SMOOTH_UNION), \
    SDF_KO(SDF_PRIM_BOX, SDF_OP_SMOOTH_UNION), SDF_KO(SDF_PRIM_TORUS, SDF_OP_SMOOTH_UNION), \
    SDF_KO(SDF_PRIM_CAPSULE, SDF_OP_SMOOTH_UNION),                                 \
    SDF_KO(SDF_PRIM_CYLINDER, SDF_OP_SMOOTH_UNION),                                \
    SDF_KO(SDF_PRIM_ROUND_BOX, SDF_OP_SMOOTH_UNION),                               \
    SDF_KO(SDF_PRIM_SPHERE, SDF_OP_SMOOTH_UNION))

// ---- exact bounding-volume culling -----------------------------------------
// For op UNION, min(d, s) == d whenever s >= d; for SMOOTH_UNION,
// smin(d, s, k) == d bit for bit whenever s >= d + k (h = 0).  Every SDF here
// is exact, so s >= |p - c| - R for a sphere (c, R) containing the primitive.
// A primitive can therefore be skipped -- without changing any output bit --
// at points where |p - c| * (1 - kCullRel) >= d + k + R + kCullAbs; the
// margins cover fp32 rounding of s and of the bound.  A plane is unbounded;
// a hard-union sphere costs no more than its own bound.
constexpr float kCullAbs = 1e-4f;
constexpr float kCullRel = 1e-5f;
constexpr float kCullScale = 1.0f / (1.0f - kCullRel);
// path lengths used by cached bounds are scaled up by this factor so that
// unit directions normalised in fp32 (|dir| <= 1 + 2^-22) stay conservative
constexpr float kPathScale = 1.000002f;
constexpr bool cullable(int kind, int op) {
  return kind != SDF_PRIM_PLANE && kind != kPrimPlaneY &&
         (op == SDF_OP_SMOOTH_UNION || (op == SDF_OP_UNION && kind != SDF_PRIM_SPHERE));
}

enum SceneVariant : int {
  kVariantGeneric = 0,
  kVariantBulb = 100,
};

}  // namespace sdf
