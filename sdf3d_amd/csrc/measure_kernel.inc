// measure_kernel.inc -- integral measures of the solid (sdf_abi.h "Measures":
// sdf_measure).  Included by render_kernel.inc inside namespace SDF_NS, after
// the meshes: the sample value is Scene::eval and the owner Scene::owner_fold,
// exactly as sdf_sample and the queries call them; only the sums are new.
//
// One wave per brick of 8 x 8 x 8 cells, the mesh's bricks in the mesh's
// numbering.  The wave walks the brick's eight 8 x 8 slices, lane = sample (l1 =
// lane >> 3, l0 = lane & 7), one sample per cell at the cell's centre, so the
// ballot of "inside" is one 64-bit word, as in mesh_count, and every moment of
// the slice is a popcount of that word against a constant bit pattern: the three
// bit planes of l0 and of l1 give the first moments, their pairs l0 l0, l1 l1
// and l0 l1.  The word is wave-uniform, so those popcounts are scalar
// instructions beside the vector unit's distance evaluation.  A brick's local
// moments are shifted by its first cell (8 b_c) once, in 64 bits.
//
// The launch is grid-stride over at most kMeasureMaxBlocks workgroups of one
// wave (kernel_args.h).  A workgroup keeps its rows in LDS across its bricks --
// lane j < 16 holds slot j of a row, so adding a brick is one read and one
// write of 64 bits per lane -- and stores them once, as its record of the
// workspace; measure_reduce (mesh.hip) combines the records.  The sums are
// integers, so any order gives the same bits; nothing is atomic and nothing
// needs zeroing.
//
// Skipping a brick: MeasureArgs::skip is MeshArgs::skip (sdf_abi.cpp
// mesh_skip_bound, unchanged), tested at the mesh's centre point, lattice point
// 8 b + 4.  The proof in mesh_kernel.inc covers every point p~ within R (half
// the brick's diagonal) of the centre, as a real point, whose fp32 coordinates
// are within 2 ulp(M) of the real ones.  A cell centre of the brick is such a
// point: as a real point origin + (i + 1/2) cell lies inside the brick, and the
// kernel's RN(origin + RN(((float)i + 0.5f) cell)) has the lattice points' two
// roundings and no third, because (float)i + 0.5f is exact below 2^23 (n[c] <=
// 65536).  So when |RN(f~(c~) - iso)| > skip every sample of the brick has the
// centre's sign and none is zero: a brick proven outside contributes nothing,
// and a brick proven inside contributes the sums over its index box inside the
// grid, which have closed forms.  With owners a brick proven inside is
// evaluated: owners vary inside it.
//
// With owners the slice's inside word is split by owner: a uniform loop over
// the primitives (prim_count iterations, one for a Mandelbulb) takes the ballot
// of "inside and owner == k" and adds its moments to row 1 + k of the LDS table.
//
// Every loop bound is a constant, an argument or derived from them; no address
// depends on a sampled value.

// sample (i0, i1, i2): RN(origin + RN(((float)i + 0.5f) cell)) per axis
__device__ __forceinline__ V3 measure_point(const KARG MeasureArgs& M, int i0, int i1, int i2) {
  return mk(M.origin[0] + ((float)i0 + 0.5f) * M.cell[0], M.origin[1] + ((float)i1 + 0.5f) * M.cell[1],
            M.origin[2] + ((float)i2 + 0.5f) * M.cell[2]);
}
// the mesh's lattice point (mesh_point): the centre of a brick
__device__ __forceinline__ V3 measure_lattice_point(const KARG MeasureArgs& M, int i0, int i1, int i2) {
  return mk(M.origin[0] + (float)i0 * M.cell[0], M.origin[1] + (float)i1 * M.cell[1],
            M.origin[2] + (float)i2 * M.cell[2]);
}

// The moments of a set of samples in coordinates local to a box (a brick, or
// one slice of it): small integers.  `any` is the union of the slices' words.
struct MeasureLocal {
  int n, a0, a1, a2, q00, q11, q22, q01, q02, q12;
  unsigned long long any;
  int zlo, zhi;   // first and last l2 with a sample (8, -1: none)
};
__device__ __forceinline__ MeasureLocal measure_local_zero() {
  return MeasureLocal{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0ull, 8, -1};
}
__device__ __forceinline__ int mpop(unsigned long long m) { return __builtin_popcountll(m); }
// slice l2 with the inside word m (bit l1 * 8 + l0)
__device__ __forceinline__ void measure_slice(MeasureLocal& L, unsigned long long m, int l2) {
  constexpr unsigned long long X0 = 0xAAAAAAAAAAAAAAAAull, X1 = 0xCCCCCCCCCCCCCCCCull,
                               X2 = 0xF0F0F0F0F0F0F0F0ull;   // the bit planes of l0
  constexpr unsigned long long Y0 = 0xFF00FF00FF00FF00ull, Y1 = 0xFFFF0000FFFF0000ull,
                               Y2 = 0xFFFFFFFF00000000ull;   // and of l1
  const unsigned long long x0 = m & X0, x1 = m & X1, x2 = m & X2;
  const unsigned long long y0 = m & Y0, y1 = m & Y1, y2 = m & Y2;
  const int n = mpop(m);
  const int px0 = mpop(x0), px1 = mpop(x1), px2 = mpop(x2);
  const int py0 = mpop(y0), py1 = mpop(y1), py2 = mpop(y2);
  const int a0 = px0 + 2 * px1 + 4 * px2;
  const int a1 = py0 + 2 * py1 + 4 * py2;
  // (b0 + 2 b1 + 4 b2)^2 = b0 + 4 b1 + 16 b2 + 4 b0 b1 + 8 b0 b2 + 16 b1 b2
  const int q00 = px0 + 4 * px1 + 16 * px2 + 4 * mpop(x0 & X1) + 8 * mpop(x0 & X2) + 16 * mpop(x1 & X2);
  const int q11 = py0 + 4 * py1 + 16 * py2 + 4 * mpop(y0 & Y1) + 8 * mpop(y0 & Y2) + 16 * mpop(y1 & Y2);
  const int q01 = (mpop(x0 & Y0) + 2 * mpop(x0 & Y1) + 4 * mpop(x0 & Y2)) +
                  2 * (mpop(x1 & Y0) + 2 * mpop(x1 & Y1) + 4 * mpop(x1 & Y2)) +
                  4 * (mpop(x2 & Y0) + 2 * mpop(x2 & Y1) + 4 * mpop(x2 & Y2));
  L.n += n;
  L.a0 += a0;
  L.a1 += a1;
  L.a2 += l2 * n;
  L.q00 += q00;
  L.q11 += q11;
  L.q22 += l2 * l2 * n;
  L.q01 += q01;
  L.q02 += l2 * a0;
  L.q12 += l2 * a1;
  L.any |= m;
  L.zlo = (m != 0ull && l2 < L.zlo) ? l2 : L.zlo;
  L.zhi = (m != 0ull && l2 > L.zhi) ? l2 : L.zhi;
}

// A row's sixteen slots as what one set contributes (sdf_abi.h "Measures").
struct MeasureRow {
  long long s[SDF_MEASURE_SLOTS];
};
// the empty set of the grid: the row every table row starts from
__device__ __forceinline__ MeasureRow measure_empty(const KARG MeasureArgs& M) {
  MeasureRow r;
#pragma unroll
  for (int j = 0; j < kMeasureSums; j++) r.s[j] = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    r.s[kMeasureLo + c] = M.n[c];
    r.s[kMeasureHi + c] = -1;
  }
  return r;
}
// local moments in a box whose first cell is (c0, c1, c2), as the grid's
__device__ __forceinline__ MeasureRow measure_shift(const KARG MeasureArgs& M, const MeasureLocal& L,
                                                    int c0, int c1, int c2) {
  MeasureRow r = measure_empty(M);
  const long long n = L.n, C0 = c0, C1 = c1, C2 = c2;
  r.s[0] = n;
  r.s[1] = L.a0 + C0 * n;
  r.s[2] = L.a1 + C1 * n;
  r.s[3] = L.a2 + C2 * n;
  r.s[4] = L.q00 + 2 * C0 * L.a0 + C0 * C0 * n;
  r.s[5] = L.q11 + 2 * C1 * L.a1 + C1 * C1 * n;
  r.s[6] = L.q22 + 2 * C2 * L.a2 + C2 * C2 * n;
  r.s[7] = L.q01 + C0 * L.a1 + C1 * L.a0 + C0 * C1 * n;
  r.s[8] = L.q02 + C0 * L.a2 + C2 * L.a0 + C0 * C2 * n;
  r.s[9] = L.q12 + C1 * L.a2 + C2 * L.a1 + C1 * C2 * n;
  if (L.any != 0ull) {
    unsigned long long col = L.any | (L.any >> 32);   // the union of the rows: bit l0
    col |= col >> 16;
    col |= col >> 8;
    const unsigned cb = (unsigned)col & 0xffu;
    r.s[kMeasureLo + 0] = c0 + __builtin_ctz(cb);
    r.s[kMeasureHi + 0] = c0 + 31 - __builtin_clz(cb);
    r.s[kMeasureLo + 1] = c1 + (__builtin_ctzll(L.any) >> 3);
    r.s[kMeasureHi + 1] = c1 + ((63 - __builtin_clzll(L.any)) >> 3);
    r.s[kMeasureLo + 2] = c2 + L.zlo;
    r.s[kMeasureHi + 2] = c2 + L.zhi;
  }
  return r;
}
// the sums of i and of i i over c <= i < c + e
__device__ __forceinline__ long long measure_sum1(long long c, long long e) {
  return e * c + e * (e - 1) / 2;
}
__device__ __forceinline__ long long measure_sum2(long long c, long long e) {
  return e * c * c + c * e * (e - 1) + (e - 1) * e * (2 * e - 1) / 6;
}
// every sample of the box [c, c + e) inside: the closed form
__device__ __forceinline__ MeasureRow measure_box(int c0, int c1, int c2, int e0, int e1, int e2) {
  MeasureRow r;
  const long long E0 = e0, E1 = e1, E2 = e2;
  const long long s0 = measure_sum1(c0, e0), s1 = measure_sum1(c1, e1), s2 = measure_sum1(c2, e2);
  r.s[0] = E0 * E1 * E2;
  r.s[1] = s0 * E1 * E2;
  r.s[2] = s1 * E0 * E2;
  r.s[3] = s2 * E0 * E1;
  r.s[4] = measure_sum2(c0, e0) * E1 * E2;
  r.s[5] = measure_sum2(c1, e1) * E0 * E2;
  r.s[6] = measure_sum2(c2, e2) * E0 * E1;
  r.s[7] = s0 * s1 * E2;
  r.s[8] = s0 * s2 * E1;
  r.s[9] = s1 * s2 * E0;
  r.s[kMeasureLo + 0] = c0;
  r.s[kMeasureLo + 1] = c1;
  r.s[kMeasureLo + 2] = c2;
  r.s[kMeasureHi + 0] = c0 + e0 - 1;
  r.s[kMeasureHi + 1] = c1 + e1 - 1;
  r.s[kMeasureHi + 2] = c2 + e2 - 1;
  return r;
}
// Lane j < 16: slot j of a row (0 in the other lanes), written lane by lane from
// the scalar registers (v_writelane_b32; a chain of selects on the lane number
// is compiled into the row stored to scratch and one indexed load, 136 bytes of
// scratch per lane, where this form has no memory behind it).
// Precondition, of measure_add as well: the row is wave-uniform -- every lane
// holds the same sixteen values -- and the call stands in wave-uniform control
// flow.  The instruction ignores EXEC and takes its value from a scalar
// register, so from inside a divergent branch, or with a row that differs
// between lanes, every lane would silently get the first active lane's row.
__device__ __forceinline__ long long measure_pick(const MeasureRow& r) {
  int lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < SDF_MEASURE_SLOTS; j++) {
    // (this compiler has no builtin for the instruction; "s": a uniform value)
    asm("v_writelane_b32 %0, %1, %2" : "+v"(lo) : "s"((int)(r.s[j] & 0xffffffffll)), "n"(j));
    asm("v_writelane_b32 %0, %1, %2" : "+v"(hi) : "s"((int)(r.s[j] >> 32)), "n"(j));
  }
  return ((long long)hi << 32) | (long long)(unsigned)lo;
}
// slot j's combination: a sum, a minimum (lo) or a maximum (hi)
__device__ __forceinline__ long long measure_combine(int slot, long long a, long long b) {
  return slot < kMeasureLo ? a + b : slot < kMeasureHi ? (b < a ? b : a) : (b > a ? b : a);
}
// table row `row` takes the set `r`: lanes 0 .. 15, a slot each
__device__ __forceinline__ void measure_add(long long* table, int row, const MeasureRow& r, int lane) {
  const long long v = measure_pick(r);   // every lane: the lane writes are wave-wide
  if (lane < SDF_MEASURE_SLOTS) {
    long long* const t = table + row * SDF_MEASURE_SLOTS + lane;
    *t = measure_combine(lane, *t, v);
  }
}

template <class Scene, bool OWNERS>
__device__ __forceinline__ void measure_body() {
  const KARG MeasureArgs& M = *(const KARG MeasureArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = M.a;
  constexpr int kRows = measure_rows(OWNERS);
  __shared__ long long table[kRows * SDF_MEASURE_SLOTS];
  const int lane = threadIdx.x;
  const int l0 = lane & 7, l1 = lane >> 3;
  const Scene scene(A);
  {
    const long long v = measure_pick(measure_empty(M));
#pragma unroll 1
    for (int row = 0; row < kRows; row++)
      if (lane < SDF_MEASURE_SLOTS) table[row * SDF_MEASURE_SLOTS + lane] = v;
  }
  __syncthreads();
  // the owners a fold can give: every primitive of the list; a Mandelbulb's 0
  const int nowners = SDF_TU_BULB ? 1 : A.prim_count;
  long long evaluated = 0, closed = 0;
#pragma unroll 1
  for (long long brick = blockIdx.x; brick < M.nbricks; brick += gridDim.x) {
    const long long brow = brick / M.nb[0];
    const int c0 = 8 * (int)(brick - brow * M.nb[0]);
    const int c1 = 8 * (int)(brow % M.nb[1]);
    const int c2 = 8 * (int)(brow / M.nb[1]);
    // the brick's index box inside the grid
    const int r0 = M.n[0] - c0, r1 = M.n[1] - c1, r2 = M.n[2] - c2;
    const int e0 = r0 < 8 ? r0 : 8, e1 = r1 < 8 ? r1 : 8, e2 = r2 < 8 ? r2 : 8;
    if (M.skip < INFINITY) {
      // every lane evaluates the centre: one uniform value, no exchange
      const float fc = scene.eval(measure_lattice_point(M, c0 + 4, c1 + 4, c2 + 4)) - M.iso;
      if (__builtin_amdgcn_readfirstlane((int)(fabsf(fc) > M.skip))) {
        const bool in = __builtin_amdgcn_readfirstlane((int)(fc < 0.0f)) != 0;
        if (!in) continue;   // proven outside throughout
        if constexpr (!OWNERS) {
          measure_add(table, 0, measure_box(c0, c1, c2, e0, e1, e2), lane);
          closed++;
          continue;
        }
      }
    }
    evaluated++;
    const int i0 = c0 + l0, i1 = c1 + l1;
    const bool in_slice = l0 < e0 && l1 < e1;
    MeasureLocal all = measure_local_zero();
#pragma unroll 1
    for (int l2 = 0; l2 < e2; l2++) {
      const int i2 = c2 + l2;
      const V3 p = measure_point(M, i0, i1, i2);
      bool inside = false;
      if (in_slice) inside = scene.eval(p) - M.iso < 0.0f;   // a NaN or a zero is outside
      const unsigned long long m = __builtin_amdgcn_ballot_w64(inside);
      measure_slice(all, m, l2);
      if constexpr (OWNERS) {
        if (m != 0ull) {
          int w = -1;
          if (inside) w = scene.owner_fold(p);
#pragma unroll 1
          for (int k = 0; k < nowners; k++) {
            const unsigned long long mk_ = __builtin_amdgcn_ballot_w64(w == k);
            if (mk_ == 0ull) continue;
            MeasureLocal one = measure_local_zero();
            measure_slice(one, mk_, 0);
            measure_add(table, 1 + k, measure_shift(M, one, c0, c1, i2), lane);
          }
        }
      }
    }
    measure_add(table, 0, measure_shift(M, all, c0, c1, c2), lane);
  }
  __syncthreads();
  long long* const rec = M.ws + (long long)blockIdx.x * measure_record(kRows);
#pragma unroll 1
  for (int i = lane; i < kRows * SDF_MEASURE_SLOTS; i += 64) rec[i] = table[i];
  if (lane < kMeasureTail)
    rec[kRows * SDF_MEASURE_SLOTS + lane] = lane == 0 ? evaluated : lane == 1 ? closed : 0;
}

// The measure kernels' occupancy: an evaluation, a ballot and scalar popcounts,
// at the render kernel's waves per SIMD; with owners the owner fold besides.
#ifndef SDF_MEASURE_WAVES_PER_EU
#define SDF_MEASURE_WAVES_PER_EU SDF_WAVES_PER_EU
#endif
// a measure entry, built-in or run-time (jit_entry.inc): one wave per workgroup
#define SDF_MEASURE_KERNEL(name, Scene, OWNERS)              \
  SDF_KERNEL(64, SDF_MEASURE_WAVES_PER_EU)                   \
  void name(MeasureArgs args) {                              \
    (void)args;                                              \
    measure_body<Scene, OWNERS>();                           \
  }
template <class Scene, bool OWNERS>
SDF_MEASURE_KERNEL(measure, Scene, OWNERS)
