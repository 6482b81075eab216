// kmath.inc -- the math layer: kernel-argument access (KARG, KA, KF), V3,
// Seq, and the precision's arithmetic (gmin ... pmax3, length).
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

// The kernel's by-value KernelArgs lives in the kernarg segment; reading it
// through an address_space(4) pointer keeps every uniform access a scalar
// (s_load) read instead of a per-lane scratch copy of the 2.1 KB struct.
#define KARG __attribute__((address_space(4)))
typedef const KARG KernelArgs KA;
typedef const KARG float* KF;

// Culling bounds in VGPRs (fast precision: its SGPRs hold the primitive
// parameters) or as uniform kernel-argument values (exact precision: its
// longer sequences need the VGPRs -- with the bounds in them the CSG8 kernel
// spilled 68 bytes per lane at 8 waves, 170 MB of scratch writes per 4K
// launch; without, none, and C3/C4 exact run 1-21 % faster).
constexpr bool kBoundsInVgprs = !SDF_EXACT;

struct V3 {
  float x, y, z;
};

// Move a uniform value into a VGPR.  Used for values the march loops read
// rarely (culling bounds), so the SGPR file keeps the hot primitive
// parameters without spilling or re-loading them inside the loops.
__device__ __forceinline__ float to_vgpr(float x) {
  float y;
  asm volatile("v_mov_b32 %0, %1" : "=v"(y) : "s"(x));
  return y;
}

// A zero the compiler must treat as per-lane.  Indexing kernel arguments with
// it turns their loads into vector loads (global_load_dwordx4, every lane the
// same address) issued together, whose results land in VGPRs -- instead of a
// chain of scalar load / wait / v_mov per value at wave start.
__device__ __forceinline__ int lane_zero() {
  int z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
}

template <int... I>
struct Seq {};
template <int N, int... I>
struct MakeSeqImpl : MakeSeqImpl<N - 1, N - 1, I...> {};
template <int... I>
struct MakeSeqImpl<0, I...> {
  using type = Seq<I...>;
};
template <int N>
using MakeSeq = typename MakeSeqImpl<N>::type;

__device__ __forceinline__ V3 mk(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 muls(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

#if SDF_EXACT
// GLSL 4.60 select semantics (SURVEY.md Appendix A); IEEE sqrt and division.
__device__ __forceinline__ float gmin(float x, float y) { return y < x ? y : x; }
__device__ __forceinline__ float gmax(float x, float y) { return x < y ? y : x; }
// sqrt: IEEE (cr_math.h cr_sqrt: a v_rsq-based fast path proven on all 2^32
// inputs, tests/test_gpu_crmath.py); division: the compiler's IEEE sequence.
__device__ __forceinline__ float fsqrt(float x) { return crm::cr_sqrt(x); }
__device__ __forceinline__ float fdiv(float a, float b) { return a / b; }
// 1 / sqrt(x), both roundings IEEE as the oracle's 1 / SQRT(x): rcp_fast is
// the IEEE reciprocal on [2^-100, 2^100) (checked on all of it), which holds
// sqrt(x) for the only caller, the Mandelbulb's x = k3 in [1e-30, 4]
__device__ __forceinline__ float frsqrt(float x) { return crm::rcp_fast(crm::cr_sqrt(x)); }
// log correctly rounded to fp32, as the oracle's cr_logf (oracle/sdf_oracle.c),
// so exact precision does not inherit ocml's last-ulp choices: cr_math.h
// cr_log (checked on all 2^32 inputs).  pow: shade.h spec_pow (fp64, rounded
// once, as the oracle's cr_powf).
__device__ __forceinline__ float flog(float x) { return crm::cr_log(x); }
// Exact precision's divisions by Markstein's steps instead of the IEEE
// sequence (v_div_scale x2, v_rcp, 5 fma, v_div_fmas / v_div_fixup through
// VCC): correctly rounded, proven in cr_math.h, guarded to their domain.
//   normalize's three divisions, one shared reciprocal (div3): C4 exact
//     2.8-2.9 % faster than without, C5 1.3 %
//   the Mandelbulb's (p - c) / scale from the host's RN(1/scale), three
//     divisions per DE evaluation (BulbScene::local): C5 exact 10-11 % faster
//   the pixel's quad coordinates (2x+1)/W, (2y+1)/H (div_refined with the
//     host's RN(1/W), no guard: integers in range)
//   the capsule's h (sd_capsule) and the smooth-min's h (smin)
// (all bit-exact at 4K, profiles/r05_ab_exact_C4.json, r05_ab_divisions_C5.json).
// The DE's final division by dz and the shadow march's h^2 / (2 h_prev) stay
// IEEE: div_one measured no faster there (DESIGN.md Appendix A).
__device__ __forceinline__ V3 normalize(V3 a) {
  float l = fsqrt(dot(a, a));
  crm::div3(a.x, a.y, a.z, l);
  return a;
}
#else
// Hardware min/max (differ from the GLSL select only for a NaN first
// operand), 1-ulp v_sqrt, v_rcp-based division, v_rsq normalisation.
__device__ __forceinline__ float gmin(float x, float y) { return fminf(x, y); }
__device__ __forceinline__ float gmax(float x, float y) { return fmaxf(x, y); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fdiv(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float frsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float flog(float x) {
  return __builtin_amdgcn_logf(x) * 0.693147180559945f;
}
__device__ __forceinline__ V3 normalize(V3 a) {
  float r = frsqrt(dot(a, a));
  return mk(a.x * r, a.y * r, a.z * r);
}
#endif

__device__ __forceinline__ float gclamp(float x, float a, float b) { return gmin(gmax(x, a), b); }

// min / max inside the primitive SDFs (box, round box, cylinder, the
// capsule's clamp).  Exact precision: the hardware v_max_f32 / v_min_f32 /
// v_max3_f32 equal the GLSL select there: no operand is
// NaN (sdf_validate's working range keeps every coordinate, square and
// distance finite) and none is -0 -- |v| - b and sqrt(.) - r are never -0
// (x - y = -0 needs x = -0), and a max of such values is one of them -- so
// the only pairs where select and hardware differ, a NaN or (+0, -0), never
// occur.  The capsule's h = dot(pa, ba) / dot(ba, ba) may be -0; the select
// keeps -0 where the hardware gives +0, and h only enters pa - ba h, whose
// components are then +-0 alike and square to +0: the same length.
#if SDF_EXACT
__device__ __forceinline__ float hw_max(float x, float y) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ float hw_min(float x, float y) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ float hw_max3(float x, float y, float z) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}
__device__ __forceinline__ float pmax(float x, float y) { return hw_max(x, y); }
__device__ __forceinline__ float pmin(float x, float y) { return hw_min(x, y); }
__device__ __forceinline__ float pmax3(float x, float y, float z) { return hw_max3(x, y, z); }
#else
__device__ __forceinline__ float pmax(float x, float y) { return gmax(x, y); }
__device__ __forceinline__ float pmin(float x, float y) { return gmin(x, y); }
__device__ __forceinline__ float pmax3(float x, float y, float z) { return gmax(x, gmax(y, z)); }
#endif
__device__ __forceinline__ float length(V3 a) { return fsqrt(dot(a, a)); }
