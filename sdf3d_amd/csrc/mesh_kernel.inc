// mesh_kernel.inc -- isosurface extraction (sdf_abi.h "Meshes": sdf_mesh_count,
// sdf_mesh_emit).  Included by render_kernel.inc inside namespace SDF_NS, after
// the queries: the lattice value is Scene::eval, the normal trace_shape from a
// fresh culling state and the owner Scene::owner_fold, exactly as sdf_sample
// and the queries call them; only the extraction is new.
//
// One workgroup of one wave per brick of 8 x 8 x 8 cells.  The brick's 9^3
// lattice values w = f(p) - iso go to LDS; the wave then walks the brick's
// eight 8 x 8 slices, lane = cell (l1 = lane >> 3, l0 = lane & 7), so a ballot
// of "active" is one 64-bit word of the brick's activity mask and every count
// is a popcount.  mesh_count writes mask and counts, a scan (mesh.hip) turns
// the counts into offsets, mesh_emit evaluates the non-empty bricks again and
// writes the mesh: a vertex's number is offset[brick] + popcount(mask bits
// below its cell), which also resolves the cells of the three negative-side
// neighbour bricks a quad reaches into.
//
// Skipping a brick (the proof of MeshArgs::skip, computed by sdf_abi.cpp
// mesh_skip_bound).  Let F be the scene function in real arithmetic.  Every
// primitive of the scene spec is an exact distance (1-Lipschitz) except a
// plane, whose gradient is its normal n (|n|-Lipschitz); min and max keep the
// larger constant of their operands; so does the polynomial smooth-min
// smin(a, b) = min(a, b) - h^2 k / 4, h = max(k - |a - b|, 0) / k: where 0 < h
// < 1 its partial derivatives are 1 - h / 2 towards the smaller operand and
// h / 2 towards the larger, a convex combination, and the negations of the
// subtracting and intersecting forms change no norm.  F is therefore
// L-Lipschitz with L = max(1, largest |n|).  A brick's lattice points lie, as
// real points, within R (half the brick's diagonal) of its centre.  The
// kernel evaluates fp32 points p~ = RN(origin + RN(i cell)), each coordinate
// within 2 ulp(M) <= 2^-22 M of the real one (M the largest coordinate
// magnitude of the grid, brick overhang included; indices stay below 2^24, so
// (float)i is exact), and computes f~ with an error |f~(p~) - F(p~)| <= E.
// E: a primitive is at most 16 fp32 operations on values of magnitude at most
// V = 4 (M + S) max(1, S) + |iso| (S the largest parameter or blend radius;
// a capsule's h is a quotient of a dot product bounded by |v| |ba| over
// |ba|^2, so its error returns to the scale of |v|), each with relative error
// at most 2^-23 in either precision (fast: the hardware reciprocal, square
// root and reciprocal square root are good to 1 ulp), so at most 2^-19 V; a
// fold step adds at most 4 roundings of that size and passes its operands'
// errors on with total weight 1 (the convex combination above); 16
// primitives: E <= 16 (16 + 4) 2^-23 V < 2^-14 V.  Then for every lattice
// point of the brick, with c~ the computed centre,
//   |f~(p~) - f~(c~)| <= 2 E + L (R + 2 sqrt 3 2^-22 M) <= L R + 2^-13 V - 2^-15 V
// (L M <= 2 V).  The test compares t = |RN(f~(c~) - iso)|, within 2^-24 V of the
// real difference, against skip >= L R + 2^-13 V (double arithmetic, rounded
// up): when it holds, every w = RN(f~(p~) - iso) of the brick has the sign of
// f~(c~) - iso and none is zero (a difference of two floats is never rounded to
// zero), so no cell of the brick is active and none of its edges crosses -- the
// brick contributes exactly what its evaluation would: nothing.  The bound is
// a proof while M and S are at most 2^20 (no square overflows, underflow is
// negligible against 2^-13 V >= 2^-11); beyond that range, for lattice indices
// of 2^24 and more, and for the Mandelbulb, whose estimator has no Lipschitz
// bound, the host passes skip = +INF and every brick is evaluated.  kCullAbs
// is a constant and therefore a proof only near the origin (DESIGN.md
// "Culling margins at large coordinates"); this margin grows with M instead.

constexpr int kMeshLattice = 9 * 9 * 9;

// lattice point (i0, i1, i2): RN(origin + RN((float)i cell)) per axis
__device__ __forceinline__ V3 mesh_point(const KARG MeshArgs& M, int i0, int i1, int i2) {
  return mk(M.origin[0] + (float)i0 * M.cell[0], M.origin[1] + (float)i1 * M.cell[1],
            M.origin[2] + (float)i2 * M.cell[2]);
}

struct MeshBrickAt {
  long long brick;
  int c0, c1, c2;   // the brick's first cell
};
__device__ __forceinline__ MeshBrickAt mesh_brick_at(const KARG MeshArgs& M) {
  MeshBrickAt b;
  b.brick = (long long)blockIdx.x;
  const long long row = b.brick / M.nb[0];
  b.c0 = 8 * (int)(b.brick - row * M.nb[0]);
  b.c1 = 8 * (int)(row % M.nb[1]);
  b.c2 = 8 * (int)(row / M.nb[1]);
  return b;
}

// The brick's lattice into LDS: w[(l2 * 9 + l1) * 9 + l0] = RN(f(p) - iso) at
// the points inside the grid (0 beyond it: only cells beyond it read those).
// mesh_count and mesh_emit share this function, so both see the same values.
template <class Scene>
__device__ __forceinline__ void mesh_lattice(const KARG MeshArgs& M, const Scene& scene,
                                             const MeshBrickAt& b, float* w) {
#pragma unroll 1
  for (int i = threadIdx.x; i < kMeshLattice; i += 64) {
    const int l2 = i / 81, r = i - 81 * l2, l1 = r / 9, l0 = r - 9 * l1;
    const int i0 = b.c0 + l0, i1 = b.c1 + l1, i2 = b.c2 + l2;
    float v = 0.0f;
    if (i0 <= M.n[0] && i1 <= M.n[1] && i2 <= M.n[2]) v = scene.eval(mesh_point(M, i0, i1, i2)) - M.iso;
    w[i] = v;
  }
  __syncthreads();
}

// The lane's cell of slice l2: its 8 corner values (corner d0 + 2 d1 + 4 d2)
// and their inside bits (w < 0; a NaN or a zero is outside).
struct MeshCell {
  float w[8];
  unsigned in;
};
__device__ __forceinline__ MeshCell mesh_cell(const float* w, int l0, int l1, int l2) {
  MeshCell c;
  c.in = 0u;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    c.w[k] = w[((l2 + (k >> 2)) * 9 + l1 + ((k >> 1) & 1)) * 9 + l0 + (k & 1)];
    c.in |= (c.w[k] < 0.0f ? 1u : 0u) << k;
  }
  return c;
}
// edge 4a of the cell (from corner 000 along a) crosses
__device__ __forceinline__ bool mesh_edge0(unsigned in, int a) { return ((in ^ (in >> (1 << a))) & 1u) != 0; }

template <class Scene>
__device__ __forceinline__ void mesh_count_body() {
  const KARG MeshArgs& M = *(const KARG MeshArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = M.a;
  __shared__ float w[kMeshLattice];
  const int lane = threadIdx.x;
  const MeshBrickAt b = mesh_brick_at(M);
  const MeshLayout L(M.nbricks);
  unsigned long long* const mask = (unsigned long long*)(M.ws + L.mask) + 8 * b.brick;
  MeshBrick* const out = (MeshBrick*)(M.ws + L.brick) + b.brick;
  const Scene scene(A);
  if (M.skip < INFINITY) {
    // every lane evaluates the centre: one uniform value, no exchange
    const float fc = scene.eval(mesh_point(M, b.c0 + 4, b.c1 + 4, b.c2 + 4)) - M.iso;
    if (__builtin_amdgcn_readfirstlane((int)(fabsf(fc) > M.skip))) {
      if (lane < 8) mask[lane] = 0ull;
      if (lane == 0) {
        out->nv = 0u;
        out->nt = 0u;
      }
      return;
    }
  }
  mesh_lattice(M, scene, b, w);
  const int l0 = lane & 7, l1 = lane >> 3;
  const int i0 = b.c0 + l0, i1 = b.c1 + l1;
  unsigned nv = 0u, nt = 0u;
#pragma unroll 1
  for (int l2 = 0; l2 < 8; l2++) {
    const int i2 = b.c2 + l2;
    const MeshCell c = mesh_cell(w, l0, l1, l2);
    const bool valid = i0 < M.n[0] && i1 < M.n[1] && i2 < M.n[2];
    const unsigned long long m = __builtin_amdgcn_ballot_w64(valid && c.in != 0u && c.in != 255u);
    if (lane == 0) mask[l2] = m;
    nv += (unsigned)__builtin_popcountll(m);
    // edge 4a emits a quad when it crosses and the cell has neighbours below along u and v
    const bool e0 = valid && mesh_edge0(c.in, 0) && i1 >= 1 && i2 >= 1;
    const bool e1 = valid && mesh_edge0(c.in, 1) && i2 >= 1 && i0 >= 1;
    const bool e2 = valid && mesh_edge0(c.in, 2) && i0 >= 1 && i1 >= 1;
    nt += 2u * (unsigned)(__builtin_popcountll(__builtin_amdgcn_ballot_w64(e0)) +
                          __builtin_popcountll(__builtin_amdgcn_ballot_w64(e1)) +
                          __builtin_popcountll(__builtin_amdgcn_ballot_w64(e2)));
  }
  if (lane == 0) {
    out->nv = nv | kMeshEvaluated;
    out->nt = nt;
  }
}

// the vertex number of cell (i0, i1, i2), an active cell of any brick
__device__ __forceinline__ long long mesh_vertex_id(const KARG MeshArgs& M, const MeshLayout& L,
                                                    int i0, int i1, int i2) {
  const long long brick = ((long long)(i2 >> 3) * M.nb[1] + (i1 >> 3)) * M.nb[0] + (i0 >> 3);
  const unsigned long long* const mask = (const unsigned long long*)(M.ws + L.mask) + 8 * brick;
  long long id = ((const MeshOffset*)(M.ws + L.offset))[brick].v;
  const int l2 = i2 & 7;
  for (int z = 0; z < l2; z++) id += __builtin_popcountll(mask[z]);
  return id + __builtin_popcountll(mask[l2] & ((1ull << ((i1 & 7) * 8 + (i0 & 7))) - 1ull));
}

// the vertex of an active cell (sdf_abi.h "Meshes"): the mean of the cell's
// crossing-edge points in local coordinates, edges in increasing e = 4a + s + 2t
__device__ __forceinline__ V3 mesh_vertex(const KARG MeshArgs& M, const MeshCell& c, int i0, int i1,
                                          int i2) {
  float S[3] = {0.0f, 0.0f, 0.0f};
  int m = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int u = (a + 1) % 3, v = (a + 2) % 3;
#pragma unroll
    for (int st = 0; st < 4; st++) {
      const int s = st & 1, t = st >> 1;
      const int ka = (s << u) | (t << v), kb = ka | (1 << a);
      const float wa = c.w[ka], wb = c.w[kb];
      const bool cross = (((c.in >> ka) ^ (c.in >> kb)) & 1u) != 0;
      const float tau = fdiv(wa, wa - wb);
      S[a] = cross ? S[a] + tau : S[a];
      S[u] = cross ? S[u] + (float)s : S[u];
      S[v] = cross ? S[v] + (float)t : S[v];
      m += cross ? 1 : 0;
    }
  }
  const float fm = (float)m;
  const V3 p = mesh_point(M, i0, i1, i2);
  return mk(p.x + fdiv(S[0], fm) * M.cell[0], p.y + fdiv(S[1], fm) * M.cell[1],
            p.z + fdiv(S[2], fm) * M.cell[2]);
}

// v < cap for a number v that a stale workspace may have made negative
__device__ __forceinline__ bool mesh_fits(long long v, long long cap) {
  return (unsigned long long)v < (unsigned long long)cap;
}

// the two triangles of edge 4a's quad, numbers t and t + 1
__device__ __forceinline__ void mesh_quad(const KARG MeshArgs& M, const MeshLayout& L, int a,
                                          const int (&i)[3], long long self, bool inside,
                                          long long t) {
  if (!mesh_fits(t, M.max_tris)) return;
  const int u = (a + 1) % 3, v = (a + 2) % 3;
  int j[3] = {i[0], i[1], i[2]};
  j[v] -= 1;
  const long long k1 = mesh_vertex_id(M, L, j[0], j[1], j[2]);   // cell - e_v
  j[u] -= 1;
  const long long k0 = mesh_vertex_id(M, L, j[0], j[1], j[2]);   // cell - e_u - e_v
  j[v] += 1;
  const long long k3 = mesh_vertex_id(M, L, j[0], j[1], j[2]);   // cell - e_u
  const int q0 = (int)(inside ? k0 : k3), q1 = (int)(inside ? k1 : self),
            q2 = (int)(inside ? self : k1), q3 = (int)(inside ? k3 : k0);
  int32_t* const o = M.tris + 3 * t;
  o[0] = q0;
  o[1] = q1;
  o[2] = q2;
  if (mesh_fits(t + 1, M.max_tris)) {
    o[3] = q0;
    o[4] = q2;
    o[5] = q3;
  }
}

template <class Scene>
__device__ __forceinline__ void mesh_emit_body() {
  const KARG MeshArgs& M = *(const KARG MeshArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = M.a;
  __shared__ float w[kMeshLattice];
  __shared__ float vp[3 * 512];   // the brick's vertices in their order, for the second pass
  const int lane = threadIdx.x;
  const MeshBrickAt b = mesh_brick_at(M);
  const MeshLayout L(M.nbricks);
  const unsigned long long* const mask = (const unsigned long long*)(M.ws + L.mask) + 8 * b.brick;
  if ((((const MeshBrick*)(M.ws + L.brick))[b.brick].nv & ~kMeshEvaluated) == 0u) return;
  const MeshOffset off = ((const MeshOffset*)(M.ws + L.offset))[b.brick];
  const Scene scene(A);
  mesh_lattice(M, scene, b, w);
  const int l0 = lane & 7, l1 = lane >> 3;
  const unsigned long long below = (1ull << lane) - 1ull;
  long long vbase = off.v, tbase = off.t;
#pragma unroll 1
  for (int l2 = 0; l2 < 8; l2++) {
    const int i[3] = {b.c0 + l0, b.c1 + l1, b.c2 + l2};
    // the count's own mask: the numbering is the one the offsets were scanned from
    const unsigned long long m = mask[l2];
    const bool active = ((m >> lane) & 1ull) != 0;
    const MeshCell c = mesh_cell(w, l0, l1, l2);
    const long long self = vbase + __builtin_popcountll(m & below);
    if (active) {
      const V3 P = mesh_vertex(M, c, i[0], i[1], i[2]);
      float* const l = vp + 3 * (int)(self - off.v);   // at most 511: a sum of mask popcounts
      l[0] = P.x;
      l[1] = P.y;
      l[2] = P.z;
      if (mesh_fits(self, M.max_verts)) {
        float* const o = M.verts + 3 * self;
        o[0] = P.x;
        o[1] = P.y;
        o[2] = P.z;
      }
    }
    const bool e0 = active && mesh_edge0(c.in, 0) && i[1] >= 1 && i[2] >= 1;
    const bool e1 = active && mesh_edge0(c.in, 1) && i[2] >= 1 && i[0] >= 1;
    const bool e2 = active && mesh_edge0(c.in, 2) && i[0] >= 1 && i[1] >= 1;
    const unsigned long long b0 = __builtin_amdgcn_ballot_w64(e0), b1 = __builtin_amdgcn_ballot_w64(e1),
                             b2 = __builtin_amdgcn_ballot_w64(e2);
    long long t = tbase + 2 * (__builtin_popcountll(b0 & below) + __builtin_popcountll(b1 & below) +
                               __builtin_popcountll(b2 & below));
    const bool inside = (c.in & 1u) != 0;
    if (e0) {
      mesh_quad(M, L, 0, i, self, inside, t);
      t += 2;
    }
    if (e1) {
      mesh_quad(M, L, 1, i, self, inside, t);
      t += 2;
    }
    if (e2) mesh_quad(M, L, 2, i, self, inside, t);
    vbase += __builtin_popcountll(m);
    tbase += 2 * (__builtin_popcountll(b0) + __builtin_popcountll(b1) + __builtin_popcountll(b2));
  }
  // Normals and owners, 64 vertices of the brick at a time.  A slice has about
  // three active cells of its 64 (measured on C4 at 256^3: 152,554 vertices in
  // 5,955 x 8 slices), so evaluating them slice by slice would run the normal's
  // taps and the owner fold eight times per brick at a twentieth of the lanes.
  if (!M.normal && !M.prim) return;
  __syncthreads();
  const int count = (int)(vbase - off.v);
#pragma unroll 1
  for (int r = lane; r < count; r += 64) {
    const long long self = off.v + r;
    if (!mesh_fits(self, M.max_verts)) continue;
    const V3 P = mk(vp[3 * r], vp[3 * r + 1], vp[3 * r + 2]);
    if (M.normal) {
      // sdf_sample's normal at P: a fresh culling state at path length 0
      MarchState mst;
      Surface S;
      S.P = P;
      S.tP = 0.0f;
      trace_shape(A, scene, mst, S);
      float* const q = M.normal + 3 * self;
      q[0] = S.N.x;
      q[1] = S.N.y;
      q[2] = S.N.z;
    }
    if (M.prim) M.prim[self] = scene.owner_fold(P);
  }
}

// The mesh kernels' occupancy: mesh_count is an evaluation and a few ballots, at
// the render kernel's waves per SIMD; mesh_emit's 9 KB of LDS per one-wave
// workgroup (the lattice and the brick's vertices) admit 5.
#ifndef SDF_MESH_WAVES_PER_EU
#define SDF_MESH_WAVES_PER_EU SDF_WAVES_PER_EU
#endif
#ifndef SDF_MESH_EMIT_WAVES_PER_EU
#define SDF_MESH_EMIT_WAVES_PER_EU 5
#endif
template <class Scene, int EMIT>
__device__ __forceinline__ void mesh_body() {
  if constexpr (EMIT) mesh_emit_body<Scene>();
  else mesh_count_body<Scene>();
}
template <class Scene>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SDF_MESH_WAVES_PER_EU, SDF_MESH_WAVES_PER_EU)))
void mesh_count(MeshArgs args) {
  (void)args;
  mesh_count_body<Scene>();
}
template <class Scene>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SDF_MESH_EMIT_WAVES_PER_EU, SDF_MESH_EMIT_WAVES_PER_EU)))
void mesh_emit(MeshArgs args) {
  (void)args;
  mesh_emit_body<Scene>();
}
