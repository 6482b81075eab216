// render_entry.inc -- the render family's entries: the supersampling resolve,
// render_body, the render kernels and the persistent render_frames.
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

// ---- supersampling resolve (sdf_abi.h sdf_params.samples) ------------------
// The wave's 8x8 tile holds whole S x S groups of sub-samples (S = 2 or 4, a
// uniform): lane bits 0, 1 carry a sub-sample's x inside the tile and bits 3,
// 4 its y.  One channel's group sum in the contract's order -- a balanced
// pairwise tree, first along x, then along y, left / lower operand first:
//   S = 2   h_j = c[0][j] + c[1][j];                      (h_0 + h_1)
//   S = 4   a_j = (c[0][j] + c[1][j]) + (c[2][j] + c[3][j]);
//           (a_0 + a_1) + (a_2 + a_3)
// by adding the xor-partner's value (wave_bits.h: DPP quad_perm for 1 and 2,
// ds_swizzle for 8 and 16).  The group's (0, 0) lane is the left / lower
// operand of every addition it makes, so it ends with the tree's value; the
// other lanes' sums are not used.  Plain fp32 additions, never fused.
// (The exchanges for 8 and 16 as VALU moves instead -- DPP row_ror:8 and
// v_permlane16_swap -- measured no faster, DESIGN.md: the LDS round trips at
// the wave's end are not what the epilogue costs.)
__device__ __forceinline__ float ssaa_sum(float v, bool four) {
#pragma clang fp contract(off)
  v = v + __uint_as_float(xor_partner<1>(__float_as_uint(v)));
  if (four) v = v + __uint_as_float(xor_partner<2>(__float_as_uint(v)));
  v = v + __uint_as_float(xor_partner<8>(__float_as_uint(v)));
  if (four) v = v + __uint_as_float(xor_partner<16>(__float_as_uint(v)));
  return v;
}

// TILES: the output is the TILES wire format (a separate instantiation, so
// the encoder's registers never weigh on the plain-format kernels)
// SSAA: the lanes are the sub-samples of a supersampled frame and the output
// is their resolved pixels (render_ssaa, an instantiation of its own as well)
// LIGHTS: the pixel's colour is the sum over the launch's lights
// (shade_pixel_lights; render_lights, instantiations of their own)
// MATERIALS (with LIGHTS): a material per primitive, blended at P
// (shade_pixel_materials; render_materials, instantiations of their own)
// REFLECT (with LIGHTS; MATERIALS: the scene has a primitive list to fold
// over): the pixel's path of mirror bounces (shade_pixel_reflect;
// render_reflect, instantiations of their own)
// ENV (with REFLECT): the path with a sky for missed layers and distance fog
// (shade_pixel_env; render_env, instantiations of their own)
template <class Scene, bool TILES, bool STEPS, bool SSAA = false, bool LIGHTS = false,
          bool MATERIALS = false, bool REFLECT = false, bool ENV = false>
__device__ __forceinline__ void render_body() {
  static_assert(!(TILES && SSAA), "a TILES stream carries shading terms, not colours");
  static_assert(!(TILES && LIGHTS), "a TILES stream carries one light's terms");
  static_assert(LIGHTS || !MATERIALS, "the materials kernels are lights kernels");
  static_assert(LIGHTS || !REFLECT, "the reflect kernels are lights kernels");
  static_assert(REFLECT || !ENV, "the env kernels are reflect kernels");
  const KARG char* const seg = (const KARG char*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = *(KA*)seg;
  const KARG RowOrder& O = *(const KARG RowOrder*)(seg + __builtin_offsetof(RenderArgs, o));
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int x = blockIdx.x * (8 * kWgWaves) + wave * 8 + (lane & 7);
  // the packed 8-row block of this row of workgroups: a schedule's order
  // (kernel_args.h RowOrder: the costliest blocks of earlier frames first),
  // else bottom-up (static middle-out and top-down orders measured slower on
  // C3/C4, profiles/r04_ab_row_order.json)
  const int by = O.n > 0 ? (int)O.order[blockIdx.y] : (int)blockIdx.y;
  const unsigned long long t_start = O.cost ? __builtin_amdgcn_s_memtime() : 0ull;
  const int pr = by * 8 + (lane >> 3);
  const bool valid = x < A.width && pr < A.rows;
  if constexpr (!TILES) {
    // SSAA: a group of S x S sub-samples leaves whole or not at all.  The
    // tile starts at multiples of 8 in x and in packed rows and 8 is a
    // multiple of S, so a group never straddles a wave; A.width = S W and
    // A.rows = S rows are multiples of S, and so is every run of packed rows
    // (block_rows and the frame's last row are S times the request's), so a
    // group lies wholly inside or wholly outside the frame and inside one
    // tiling block: its lanes share `valid` and consecutive frame rows, and
    // the resolve below exchanges values among lanes that are all present.
    if (!valid) return;
  } else {
    // every lane of a wave with a pixel in the frame stays: the tile encoder
    // is a wave-wide operation (store_tiles)
    if (blockIdx.x * kWgWaves + wave >= ((A.width + 7) >> 3)) return;
  }
  // packed row -> frame row: period blk, row `within` of its run of blocks.
  // A run of a multiple of 8 rows (every tiling of 8-row blocks) holds the
  // wave's 8 packed rows whole: its period and offset are wave-uniform,
  // scalar arithmetic (the per-lane integer division was ~20 VALU per wave,
  // tools/block_counts.py)
  int y;
  const int r0 = by * 8;
  if ((A.chunk_rows & 7) == 0) {
    const int blk0 = r0 / A.chunk_rows;
    y = (A.first_block + blk0 * A.block_stride) * A.block_rows + (r0 - blk0 * A.chunk_rows) +
        (lane >> 3);
  } else {
    const int blk = pr / A.chunk_rows;
    const int within = pr - blk * A.chunk_rows;
    y = (A.first_block + blk * A.block_stride) * A.block_rows + within;
  }
  if (A.run_gap_rows) {
    // spaced runs (sdf_tiling.run_step): block_rows % 8 == 0, so the wave's
    // 8 packed rows lie in one block, found with scalar arithmetic
    const int w0 = r0 - (r0 / A.chunk_rows) * A.chunk_rows;
    y += (w0 / A.block_rows) * A.run_gap_rows;
  }
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
  int sp = 0, ss = 0;
  if (valid) {
    const Scene scene(A);
    if constexpr (LIGHTS) {
      const KARG LightsArgs& L =
          *(const KARG LightsArgs*)(seg + __builtin_offsetof(RenderArgs, l));
      if constexpr (REFLECT) {
        const KARG MaterialArgs& M =
            *(const KARG MaterialArgs*)(seg + __builtin_offsetof(RenderArgs, m));
        const KARG ReflectArgs& R =
            *(const KARG ReflectArgs*)(seg + __builtin_offsetof(RenderArgs, r));
        if constexpr (ENV) {
          const KARG EnvArgs& E =
              *(const KARG EnvArgs*)(seg + __builtin_offsetof(RenderArgs, e));
          c = shade_pixel_env<STEPS, MATERIALS>(A, L, M, R, E, scene, ArgsView{A}, x, y, sp, ss);
        } else {
          c = shade_pixel_reflect<STEPS, MATERIALS>(A, L, M, R, scene, ArgsView{A}, x, y, sp,
                                                    ss);
        }
      } else if constexpr (MATERIALS) {
        const KARG MaterialArgs& M =
            *(const KARG MaterialArgs*)(seg + __builtin_offsetof(RenderArgs, m));
        c = shade_pixel_materials<STEPS>(A, L, M, scene, ArgsView{A}, x, y, sp, ss);
      } else {
        c = shade_pixel_lights<STEPS>(A, L, scene, ArgsView{A}, x, y, sp, ss);   // the colour
      }
    } else {
      c = shade_pixel<STEPS>(A, scene, ArgsView{A}, x, y, sp, ss);
    }
  }
  const size_t o = (size_t)(A.frame_rows ? y : pr) * A.width + x;
  if (O.cost) {
    // this wave's cycles to its block (one lane: a vector atomic)
    const unsigned long long dt = __builtin_amdgcn_s_memtime() - t_start;
    if (lane == (int)__builtin_ctzll(__builtin_amdgcn_read_exec()))
      atomicAdd(O.cost + by, dt);
  }
  if constexpr (TILES) {
    // the stream carries the shading terms (shade.h)
    const int tiles_x = (A.width + 7) >> 3;
    const int tile = by * tiles_x + blockIdx.x * kWgWaves + wave;
    store_tiles(A.rgba, tiles_x * ((A.rows + 7) >> 3), tile, lane, valid, c);
    if (tile == 0) store_tiles_shade(A.rgba, frame_shade(A), lane);
  } else if constexpr (SSAA) {
    // every lane's colour, the group sums in the contract's tree order, and
    // the group's (0, 0) lane scales by 1 / S^2 (a power of two: one
    // rounding, denormals kept), converts and writes the output pixel
    float4 s = c;
    if constexpr (!LIGHTS) s = shade_colour<SDF_EXACT>(frame_shade(A), c.x, c.y, c.z);
    const int lg = A.ss_log2;
    const bool four = lg == 2;
    const float sx = ssaa_sum(s.x, four), sy = ssaa_sum(s.y, four), sz = ssaa_sum(s.z, four);
    const int sub = (1 << lg) - 1;
    if ((lane & sub) == 0 && ((lane >> 3) & sub) == 0) {
      const float w = four ? 0.0625f : 0.25f;
      const size_t oo = (size_t)((A.frame_rows ? y : pr) >> lg) * A.out_width + (x >> lg);
      store_pixel(A.format, A.rgba, oo, make_float4(sx * w, sy * w, sz * w, 1.0f));
    }
  } else if constexpr (LIGHTS) {
    store_pixel(A.format, A.rgba, o, c);
  } else {
    store_pixel(A.format, A.rgba, o, pixel_value(A, A.format, c));
  }
  if constexpr (STEPS) {
    if (A.steps && valid) reinterpret_cast<int2*>(A.steps)[o] = make_int2(sp, ss);
  }
}

// ---- the render kernels -------------------------------------------------------
// A render kernel is render_body of its features, built at the occupancy of
// the last feature that is on (a plain one at SDF_WAVES_PER_EU): first the
// features' occupancies, then the rule (render_waves) and the one statement
// of a render entry (SDF_RENDER_KERNEL), then the built-in kernels.

// the multi-light instantiations (sdf_render_lights; the count and the colour
// flag are uniforms), with and without step recording and the supersampling
// resolve.  P, N, ao, the channel sums and a copy of the culling state live
// across the loop over the lights on top of a shadow march's registers, so
// these kernels take an occupancy of their own (DESIGN.md, Lights)
// (CSG8: 79 VGPRs fast, which 6 waves per SIMD hold; exact spilled 32 bytes
// per lane there and takes 5)
#ifndef SDF_LIGHTS_WAVES_PER_EU
#define SDF_LIGHTS_WAVES_PER_EU (SDF_EXACT ? 5 : 6)
#endif

// the per-primitive material instantiations (sdf_render_materials): the
// lights kernels with the material fold at P between the surface and the
// lights (shade_pixel_materials); the fold's nine running components are dead
// before the first shadow march, where the blended dif and ref (6 VGPRs) stay
// live instead of uniform ones (DESIGN.md, Materials: the register figures
// and the choice of occupancy)
// (CSG8 exact: 96 VGPRs at the lights kernels' 5 waves per SIMD, no scratch.
// CSG8 fast at their 6 waves: 80 VGPRs and 20-28 bytes of scratch per lane,
// stored once before the loop over the lights and read back after it, one
// dword per light inside it, none in a march; at 5 waves 87-90 VGPRs without
// scratch, measured slower by about half a percent (1 light) and one percent
// (4 lights) on C4 at 1080p (profiles/materials_C4.json, materials_w5), so 6
// stays)
#ifndef SDF_MATERIALS_WAVES_PER_EU
#define SDF_MATERIALS_WAVES_PER_EU SDF_LIGHTS_WAVES_PER_EU
#endif

// the reflect instantiations (sdf_render_reflect): the materials kernels'
// pixel inside a loop over the path's layers (shade_pixel_reflect).  The next
// ray, the weights, the composite and the step sums live across a whole layer
// on top of the materials kernel's registers, so these kernels take an
// occupancy of their own (DESIGN.md, Reflections: the register figures)
#ifndef SDF_REFLECT_WAVES_PER_EU
#define SDF_REFLECT_WAVES_PER_EU 4
#endif

// the env instantiations (sdf_render_env): the reflect kernels' path with the
// miss test between a layer's march and its surface work (shade_pixel_env),
// at the reflect kernels' occupancy (DESIGN.md, Environment: the register
// figures)
#ifndef SDF_ENV_WAVES_PER_EU
#define SDF_ENV_WAVES_PER_EU SDF_REFLECT_WAVES_PER_EU
#endif

// the occupancy of the last feature that is on (each feature has the ones
// before it, render_body's assertions)
constexpr int render_waves(bool lights, bool materials, bool reflect, bool env) {
  return env         ? SDF_ENV_WAVES_PER_EU
         : reflect   ? SDF_REFLECT_WAVES_PER_EU
         : materials ? SDF_MATERIALS_WAVES_PER_EU
         : lights    ? SDF_LIGHTS_WAVES_PER_EU
                     : SDF_WAVES_PER_EU;
}
// A render entry, built-in or run-time (jit_entry.inc): render_body's
// arguments after the name.
#define SDF_RENDER_KERNEL(name, Scene, TILES, STEPS, SSAA, LIGHTS, MATERIALS, REFLECT, ENV) \
  SDF_KERNEL(SDF_WG_BOUND, render_waves(LIGHTS, MATERIALS, REFLECT, ENV))                   \
  void name(RenderArgs args) {                                                              \
    (void)args;                                                                             \
    render_body<Scene, TILES, STEPS, SSAA, LIGHTS, MATERIALS, REFLECT, ENV>();              \
  }

template <class Scene, bool TILES, bool STEPS>
SDF_RENDER_KERNEL(render, Scene, false, STEPS, false, false, false, false, false)
// the TILES instantiation at the plain kernel's occupancy (8 waves per SIMD):
// its encoder epilogue would otherwise hold it to 7
template <class Scene, bool TILES, bool STEPS>
SDF_RENDER_KERNEL(render_tiles, Scene, true, STEPS, false, false, false, false, false)
// the supersampling instantiation (sdf_params.samples = 2 or 4, a uniform
// read from the arguments): the plain kernel's pixels as sub-samples, with
// the resolve epilogue; with and without step recording like `render`, so a
// sub-sample is bit for bit the pixel the plain kernel of the same STEPS
// writes for the S W x S H frame
template <class Scene, bool STEPS>
SDF_RENDER_KERNEL(render_ssaa, Scene, false, STEPS, true, false, false, false, false)
template <class Scene, bool STEPS, bool SSAA>
SDF_RENDER_KERNEL(render_lights, Scene, false, STEPS, SSAA, true, false, false, false)
template <class Scene, bool STEPS, bool SSAA>
SDF_RENDER_KERNEL(render_materials, Scene, false, STEPS, SSAA, true, true, false, false)
template <class Scene, bool STEPS, bool SSAA, bool FOLD>
SDF_RENDER_KERNEL(render_reflect, Scene, false, STEPS, SSAA, true, FOLD, true, false)
template <class Scene, bool STEPS, bool SSAA, bool FOLD>
SDF_RENDER_KERNEL(render_env, Scene, false, STEPS, SSAA, true, FOLD, true, true)

// The persistent frame-sequence kernel (sdf_render_frames): every wave
// builds its scene registers once, then renders 8x8 tiles (item = frame *
// tiles_per_frame + tile, row-major), `chunk` consecutive items per
// request to its workgroup's work queue; queue q hands out the chunks q,
// q + queues, q + 2 queues, ...  A wave asks for its next chunk while it
// renders the current one, and ends on the first chunk past the end, so the
// grid drains whatever its size (every queue has at least one workgroup).
// A tile's pixels come from the same shade_pixel as sdf_render's: identical
// frames.
template <bool STEPS, class Scene>
__device__ __forceinline__ void frames_tile(KA& A, const KARG FramesArgs& FA, const Scene& scene,
                                            uint32_t item, int lane) {
  const uint32_t per_frame = (uint32_t)FA.tiles_per_frame;
  const uint32_t f = item / per_frame;
  const uint32_t t = item - f * per_frame;
  const uint32_t ty = t / (uint32_t)FA.tiles_x;
  const int x = (int)(t - ty * (uint32_t)FA.tiles_x) * 8 + (lane & 7);
  const int y = (int)ty * 8 + (lane >> 3);
  if (x < A.width && y < A.height) {
    const FrameView V{FA.frame[f]};
    int sp = 0, ss = 0;
    const float4 c = shade_pixel<STEPS>(A, scene, V, x, y, sp, ss);
    const size_t o = (size_t)y * A.width + x;
    store_pixel(A.format, V.rgba(), o, pixel_value(A, A.format, c));
    if constexpr (STEPS) {
      if (V.steps()) reinterpret_cast<int2*>(V.steps())[o] = make_int2(sp, ss);
    }
  }
}

// the persistent frames kernel's occupancy: its queue state on top of the
// pixel's (CSG8 exact at 8 waves/SIMD spilled 156-160 bytes per lane)
#ifndef SDF_FRAMES_WAVES_PER_EU
#define SDF_FRAMES_WAVES_PER_EU SDF_WAVES_PER_EU
#endif
template <class Scene, bool STEPS>
SDF_KERNEL(256, SDF_FRAMES_WAVES_PER_EU)
void render_frames(FramesArgs args) {
  (void)args;
  const KARG FramesArgs& FA = *(const KARG FramesArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
  KA& A = FA.a;
  const int lane = threadIdx.x & 63;
  const Scene scene(A);
  const uint32_t total = (uint32_t)FA.nframes * (uint32_t)FA.tiles_per_frame;
  if (FA.schedule == 1) {
    // static: wave w takes items w, w + W, w + 2 W, ... (W waves in the grid)
    const uint32_t W = gridDim.x * (blockDim.x >> 6);
    for (uint32_t item = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); item < total;
         item += W)
      frames_tile<STEPS>(A, FA, scene, __builtin_amdgcn_readfirstlane(item), lane);
    return;
  }
  const uint32_t nq = (uint32_t)FA.queues;
  const uint32_t q = blockIdx.x % nq;
  uint32_t* const counter = FA.counter + q * kQueueStride;
  const uint32_t ck = (uint32_t)FA.chunk;
  const uint32_t chunks = (total + ck - 1) / ck;
  uint32_t next = 0u;
  if (lane == 0) next = atomicAdd(counter, 1u);
  for (;;) {
    const uint32_t chunk = __builtin_amdgcn_readfirstlane(next) * nq + q;
    if (chunk >= chunks) break;
    if (lane == 0) next = atomicAdd(counter, 1u);
#pragma unroll 1
    for (uint32_t i = chunk * ck; i < chunk * ck + ck && i < total; ++i)
      frames_tile<STEPS>(A, FA, scene, i, lane);
  }
}
