// mesh_kernel.inc -- isosurface extraction (sdf_abi.h "Meshes": sdf_mesh_count,
// sdf_mesh_emit; "Sharp meshes": sdf_mesh_emit_sharp, further down).  Included by
// render_kernel.inc inside namespace SDF_NS, after the queries and the
// gradients: the lattice value is Scene::eval, the normal trace_shape from a
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

#if !SDF_TU_BULB
// ---- sharp-feature vertices (sdf_abi.h "Sharp meshes": sdf_mesh_emit_sharp) ----
// mesh_emit with another vertex: the cell's crossings are refined along their
// edges (regula falsi on Scene::eval, the lattice's own evaluator), each gets the
// scene's analytic gradient (grad_kernel.inc grad_fold / grad_sweep: the generic
// fold of sdf_sample_grad), and the vertex is fitted to those tangent planes.
//
// A slice has about three active cells of 64, and a lattice edge is shared by
// four cells, so edges are refined per brick and not per cell.  The brick is
// taken in two slabs of kSharpSlab = 4 cell slices (5 lattice planes, the
// middle plane's edges twice, to the same bits):
//   1. the slab's 1044 lattice edges, 64 at a time, lane = edge: the crossing
//      ones inside the grid are queued in LDS in slot order (ballot, popcount);
//   2. the queue, 64 at a time, lane = crossing: `refine` evaluations, one
//      gradient, (tau, n) to the edge's slot in LDS;
//   3. the slab's four slices as in mesh_emit, lane = cell, the vertex fitted
//      from the slots of the cell's crossing edges.
// Every loop count is a constant, an argument or a popcount of sign ballots, as
// mesh_emit's are; no address depends on a refined value.
//
// LDS per one-wave workgroup: lattice 2,916 B + vertices 6,144 B + slots
// 16,704 B + queue 2,088 B + the gradient's two columns 8,192 B = 36,044 B, so
// 4 workgroups per CU of 160 KiB: one wave per SIMD, and the registers of one
// (a whole brick in one slab would be 50 KB and 3 per CU; slabs of two slices
// 5 per CU at half the lanes in step 2).
constexpr int kSharpSlab = 4;
constexpr int kSharpEdgesXY = (kSharpSlab + 1) * 72;               // along 0 (and along 1) in the slab
constexpr int kSharpEdges = 2 * kSharpEdgesXY + kSharpSlab * 81;   // 1044

// the slot of the lattice edge from the slab's point (l0, l1, lp) along a
__device__ __forceinline__ int sharp_slot(int a, int l0, int l1, int lp) {
  return a == 0   ? (lp * 9 + l1) * 8 + l0
         : a == 1 ? kSharpEdgesXY + (lp * 8 + l1) * 9 + l0
                  : 2 * kSharpEdgesXY + (lp * 9 + l1) * 9 + l0;
}
struct SharpEdge {
  int a, l0, l1, lp;
};
__device__ __forceinline__ SharpEdge sharp_edge(int slot) {
  SharpEdge e;
  e.a = slot < kSharpEdgesXY ? 0 : slot < 2 * kSharpEdgesXY ? 1 : 2;
  const int s = slot - e.a * kSharpEdgesXY;
  const int plane = e.a == 2 ? 81 : 72, row = e.a == 0 ? 8 : 9;
  e.lp = s / plane;
  const int r = s - plane * e.lp;
  e.l1 = r / row;
  e.l0 = r - row * e.l1;
  return e;
}
// the edge's ends in the brick's lattice
__device__ __forceinline__ int sharp_lattice_a(const SharpEdge& e, int s0) {
  return ((s0 + e.lp) * 9 + e.l1) * 9 + e.l0;
}
__device__ __forceinline__ int sharp_lattice_step(int a) { return a == 0 ? 1 : a == 1 ? 9 : 81; }

// the edge point at tau: RN(A_a + RN(tau cell_a)) along a, A's coordinates beside it
__device__ __forceinline__ V3 sharp_point(V3 pa, int a, float step) {
  return mk(a == 0 ? pa.x + step : pa.x, a == 1 ? pa.y + step : pa.y, a == 2 ? pa.z + step : pa.z);
}

// Steps 1 and 2 for the slab whose first slice is s0: es[slot] = (tau, n) of
// every crossing edge of the slab that lies inside the grid.
template <class Scene>
__device__ __forceinline__ void sharp_edges(const KARG MeshArgs& M, const Scene& scene,
                                            const MeshBrickAt& b, const float* w, int s0,
                                            float4* es, unsigned short* queue, float* fv,
                                            float* fd) {
  KA& A = M.a;
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  __syncthreads();   // the slab before this one has been fitted
  int count = 0;
#pragma unroll 1
  for (int base = 0; base < kSharpEdges; base += 64) {
    const int slot = base + lane;
    bool cross = false;
    if (slot < kSharpEdges) {
      const SharpEdge e = sharp_edge(slot);
      const int ia = sharp_lattice_a(e, s0);
      const float wa = w[ia], wb = w[ia + sharp_lattice_step(e.a)];
      // B inside the grid (A then is): beyond it the lattice holds zeros
      const bool in_grid = b.c0 + e.l0 + (e.a == 0) <= M.n[0] && b.c1 + e.l1 + (e.a == 1) <= M.n[1] &&
                           b.c2 + s0 + e.lp + (e.a == 2) <= M.n[2];
      cross = in_grid && ((wa < 0.0f) != (wb < 0.0f));
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(cross);
    if (cross) queue[count + __builtin_popcountll(m & below)] = (unsigned short)slot;
    count += __builtin_popcountll(m);
  }
  __syncthreads();
  // a wave's lanes beyond the queue carry its last edge and store nothing, so
  // the gradient's ballots see the whole wave
#pragma unroll 1
  for (int r0 = 0; r0 < count; r0 += 64) {
    const bool live = r0 + lane < count;
    const int slot = queue[live ? r0 + lane : count - 1];
    const SharpEdge e = sharp_edge(slot);
    const int ia = sharp_lattice_a(e, s0);
    float wa = w[ia], wb = w[ia + sharp_lattice_step(e.a)];
    const V3 pa = mesh_point(M, b.c0 + e.l0, b.c1 + e.l1, b.c2 + s0 + e.lp);
    const float cell = e.a == 0 ? M.cell[0] : e.a == 1 ? M.cell[1] : M.cell[2];
    float ta = 0.0f, tb = 1.0f;
    float tau = fdiv(wa, wa - wb);
#pragma unroll 1
    for (int k = 0; k < M.refine; k++) {
      const float wm = scene.eval(sharp_point(pa, e.a, tau * cell)) - M.iso;
      const bool same = (wm < 0.0f) == (wa < 0.0f);
      ta = same ? tau : ta;
      wa = same ? wm : wa;
      tb = same ? tb : tau;
      wb = same ? wb : wm;
      tau = ta + (tb - ta) * fdiv(wa, wa - wb);
    }
    const V3 p = sharp_point(pa, e.a, tau * cell);
    (void)grad_fold<64>(A, p, true, fv + lane, fd + lane);
    const V3 n = grad_sweep<64>(A, p, 1.0f, fv + lane, fd + lane,
                                [](int, float, float, const float (&)[7]) {});
    if (live) es[slot] = make_float4(tau, n.x, n.y, n.z);
  }
  __syncthreads();
}

// The sharp vertex of an active cell (sdf_abi.h "Sharp meshes"): mesh_vertex's
// mass point g from the refined tau, then `iterations` descent steps on the
// tangent planes of the cell's crossing edges, clamped to the cell.  (l0, l1,
// lp) is the cell in its slab.
__device__ __forceinline__ V3 mesh_vertex_sharp(const KARG MeshArgs& M, const MeshCell& c, int i0,
                                                int i1, int i2, const float4* es, int l0, int l1,
                                                int lp) {
  float S[3] = {0.0f, 0.0f, 0.0f};
  float4 E[12];
  int m = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int u = (a + 1) % 3, v = (a + 2) % 3;
#pragma unroll
    for (int st = 0; st < 4; st++) {
      const int s = st & 1, t = st >> 1;
      const int ka = (s << u) | (t << v), kb = ka | (1 << a);
      const bool cross = (((c.in >> ka) ^ (c.in >> kb)) & 1u) != 0;
      int l[3] = {l0, l1, lp};
      l[u] += s;
      l[v] += t;
      E[4 * a + st] = es[sharp_slot(a, l[0], l[1], l[2])];
      S[a] = cross ? S[a] + E[4 * a + st].x : S[a];
      S[u] = cross ? S[u] + (float)s : S[u];
      S[v] = cross ? S[v] + (float)t : S[v];
      m += cross ? 1 : 0;
    }
  }
  const float fm = (float)m;
  const float g[3] = {fdiv(S[0], fm), fdiv(S[1], fm), fdiv(S[2], fm)};
  float a00 = 0.0f, a01 = 0.0f, a02 = 0.0f, a11 = 0.0f, a12 = 0.0f, a22 = 0.0f;
  float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int u = (a + 1) % 3, v = (a + 2) % 3;
#pragma unroll
    for (int st = 0; st < 4; st++) {
      const int s = st & 1, t = st >> 1;
      const int ka = (s << u) | (t << v), kb = ka | (1 << a);
      const bool cross = (((c.in >> ka) ^ (c.in >> kb)) & 1u) != 0;
      const float4 e = E[4 * a + st];
      float q[3];
      q[a] = e.x;
      q[u] = (float)s;
      q[v] = (float)t;
      const float r0 = (q[0] - g[0]) * M.cell[0], r1 = (q[1] - g[1]) * M.cell[1],
                  r2 = (q[2] - g[2]) * M.cell[2];
      const float be = (e.y * r0 + e.z * r1) + e.w * r2;
      a00 = cross ? a00 + e.y * e.y : a00;
      a01 = cross ? a01 + e.y * e.z : a01;
      a02 = cross ? a02 + e.y * e.w : a02;
      a11 = cross ? a11 + e.z * e.z : a11;
      a12 = cross ? a12 + e.z * e.w : a12;
      a22 = cross ? a22 + e.w * e.w : a22;
      b0 = cross ? b0 + e.y * be : b0;
      b1 = cross ? b1 + e.z * be : b1;
      b2 = cross ? b2 + e.w * be : b2;
    }
  }
  const float tr = (a00 + a11) + a22;
  const float alpha = fdiv(1.0f, tr);
  float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
#pragma unroll 1
  for (int k = 0; k < M.iterations; k++) {
    const float d0 = b0 - ((a00 * x0 + a01 * x1) + a02 * x2);
    const float d1 = b1 - ((a01 * x0 + a11 * x1) + a12 * x2);
    const float d2 = b2 - ((a02 * x0 + a12 * x1) + a22 * x2);
    x0 = x0 + alpha * d0;
    x1 = x1 + alpha * d1;
    x2 = x2 + alpha * d2;
  }
  const bool ok = tr > 0.0f && tr < INFINITY && fabsf(x0) < INFINITY && fabsf(x1) < INFINITY &&
                  fabsf(x2) < INFINITY;
  x0 = ok ? x0 : 0.0f;
  x1 = ok ? x1 : 0.0f;
  x2 = ok ? x2 : 0.0f;
  const float f0 = gclamp(g[0] + fdiv(x0, M.cell[0]), 0.0f, 1.0f);
  const float f1 = gclamp(g[1] + fdiv(x1, M.cell[1]), 0.0f, 1.0f);
  const float f2 = gclamp(g[2] + fdiv(x2, M.cell[2]), 0.0f, 1.0f);
  const V3 p = mesh_point(M, i0, i1, i2);
  return mk(p.x + f0 * M.cell[0], p.y + f1 * M.cell[1], p.z + f2 * M.cell[2]);
}
#endif  // !SDF_TU_BULB

template <class Scene, bool SHARP>
__device__ __forceinline__ void mesh_emit_body() {
  const KARG MeshArgs& M = *(const KARG MeshArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = M.a;
  __shared__ float w[kMeshLattice];
  __shared__ float vp[3 * 512];   // the brick's vertices in their order, for the second pass
#if !SDF_TU_BULB
  // the sharp kernel's own (see above); unused, and gone, in mesh_emit
  __shared__ float4 es[SHARP ? kSharpEdges : 1];
  __shared__ unsigned short queue[SHARP ? kSharpEdges : 1];
  __shared__ float fv[SHARP ? SDF_MAX_PRIMS * 64 : 1];
  __shared__ float fd[SHARP ? SDF_MAX_PRIMS * 64 : 1];
#else
  static_assert(!SHARP, "a Mandelbulb has no analytic gradient");
#endif
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
#if !SDF_TU_BULB
    if constexpr (SHARP) {
      if ((l2 & (kSharpSlab - 1)) == 0) sharp_edges(M, scene, b, w, l2, es, queue, fv, fd);
    }
#endif
    if (active) {
      V3 P;
#if !SDF_TU_BULB
      if constexpr (SHARP)
        P = mesh_vertex_sharp(M, c, i[0], i[1], i[2], es, l0, l1, l2 & (kSharpSlab - 1));
      else
#endif
        P = mesh_vertex(M, c, i[0], i[1], i[2]);
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
// workgroup (the lattice and the brick's vertices) admit 5; mesh_emit_sharp's
// 36 KB one (see there).
#ifndef SDF_MESH_WAVES_PER_EU
#define SDF_MESH_WAVES_PER_EU SDF_WAVES_PER_EU
#endif
#ifndef SDF_MESH_EMIT_WAVES_PER_EU
#define SDF_MESH_EMIT_WAVES_PER_EU 5
#endif
#ifndef SDF_MESH_SHARP_WAVES_PER_EU
#define SDF_MESH_SHARP_WAVES_PER_EU 1
#endif
// KIND: 0 mesh_count, 1 mesh_emit, 2 mesh_emit_sharp
template <class Scene, int KIND>
__device__ __forceinline__ void mesh_body() {
  if constexpr (KIND == 2) mesh_emit_body<Scene, true>();
  else if constexpr (KIND == 1) mesh_emit_body<Scene, false>();
  else mesh_count_body<Scene>();
}
constexpr int mesh_waves(int kind) {
  return kind == 2 ? SDF_MESH_SHARP_WAVES_PER_EU
         : kind == 1 ? SDF_MESH_EMIT_WAVES_PER_EU
                     : SDF_MESH_WAVES_PER_EU;
}
// a mesh entry, built-in or run-time (jit_entry.inc): one wave per workgroup
#define SDF_MESH_KERNEL(name, Scene, KIND)                   \
  SDF_KERNEL(64, mesh_waves(KIND))                           \
  void name(MeshArgs args) {                                 \
    (void)args;                                              \
    mesh_body<Scene, KIND>();                                \
  }
template <class Scene>
SDF_MESH_KERNEL(mesh_count, Scene, 0)
template <class Scene>
SDF_MESH_KERNEL(mesh_emit, Scene, 1)
#if !SDF_TU_BULB
template <class Scene>
SDF_MESH_KERNEL(mesh_emit_sharp, Scene, 2)
#endif
