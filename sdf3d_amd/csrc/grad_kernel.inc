// grad_kernel.inc -- analytic gradients of the scene function (sdf_abi.h
// "Gradients": sdf_sample_grad).  Included by render_kernel.inc inside namespace
// SDF_NS, before the meshes (whose sharp kernel takes a point's gradient from
// grad_fold / grad_sweep), in the primitive translation units and the run-time
// specialised ones (no Mandelbulb); the kernels themselves are built in only.
//
// Lane = point.  The forward fold is GenericScene::eval's own loop (prim_sdf,
// combine, every primitive, unculled), so `dist` is sdf_sample's value; it
// parks each primitive's value v_i and the running distance d_(i-1) before it
// in LDS (one column per lane, so the loops stay rolled and nothing goes to
// scratch).  The backward sweep walks the list in reverse with the adjoint g of
// the running distance: fold_partials gives dd_i/dd_(i-1), dd_i/dv_i and
// dd_i/dk, prim_partials dv/dp and dv/d(public parameter).  The scene is
// wave-uniform: it is read with scalar loads from the kernel arguments, and the
// kind / op switches are scalar branches.
//
// Conventions (the derivative of the operation sequence, reverse mode): a select
// passes the adjoint to the operand the forward comparison took, written here
// with the scene spec's own comparisons (min(x, y) = y < x ? y : x, max(x, y) =
// x < y ? y : x); |x| has derivative -1 for x < 0 and +1 otherwise; a square
// root's derivative uses the guarded reciprocal grcp (1 / len for len > 0, else
// 0), which keeps every output finite: a square root here is never denormal (its
// argument is a sum of squares, at least 2^-149), so 1 / len <= 2^75.
//
// Parameter sums (grad_prims): per primitive 8 terms exist at most (k and
// p[0..6]).  They are summed across the wave as soon as they are formed, all
// eight in one six-stage xor butterfly (wave_sum8: DPP quad_perm, ds_swizzle,
// ds_bpermute; IEEE addition is commutative, so partners hold the same bits);
// lanes 0..7 then add the eight sums into the wave's own row of fp64
// accumulators in LDS.  A wave whose lanes all
// have a zero adjoint for a primitive skips it (one ballot).  After the
// grid-stride loop the workgroup adds its waves' rows in wave order, rounds once
// to fp32 and writes one row of the workspace; grad_reduce sums the rows in
// index order in fp64 and rounds once.  Nothing is atomic: the order is fixed by
// (n, grid), so equal inputs give equal bits.  Without grad_prims (PRIMS =
// false) none of that is compiled in.

constexpr int kGradWaves = kGradBlock / 64;

__device__ __forceinline__ float grcp(float x) {
#if SDF_EXACT
  return x > 0.0f ? 1.0f / x : 0.0f;
#else
  return x > 0.0f ? __builtin_amdgcn_rcpf(x) : 0.0f;
#endif
}
__device__ __forceinline__ float gsign(float x) { return x < 0.0f ? -1.0f : 1.0f; }

// The partials of one fold step d_i = combine(op, d, v, k): (a, b) as
// material_step forms them, h the smooth-min's own h in this precision's form.
//   gd = dd_i/dd, gv = dd_i/dv, gk = dd_i/dk
__device__ __forceinline__ void fold_partials(int op, float d, float v, float k4, float ik,
                                              float& gd, float& gv, float& gk) {
  const bool smooth =
      op == SDF_OP_SMOOTH_UNION || op == SDF_OP_SMOOTH_SUBTRACT || op == SDF_OP_SMOOTH_INTERSECT;
  const bool uni = op == SDF_OP_UNION || op == SDF_OP_SMOOTH_UNION;
  const bool sub = op == SDF_OP_SUBTRACT || op == SDF_OP_SMOOTH_SUBTRACT;
  const float a = uni ? d : -d;
  const float b = (op == SDF_OP_INTERSECT || op == SDF_OP_SMOOTH_INTERSECT) ? -v : v;
  const bool nearer = b < a;
  float ma = nearer ? 0.0f : 1.0f;
  gk = 0.0f;
  if (smooth) {
#if SDF_EXACT
    (void)ik;
    const float k = 4.0f * k4;
    const float h = gmax(k - fabsf(a - b), 0.0f) / k;
#else
    (void)k4;
    const float h = fminf(fmaxf(fmaf(-fabsf(a - b), ik, 1.0f), 0.0f), 1.0f);
#endif
    const float hh = 0.5f * h;
    ma = nearer ? hh : 1.0f - hh;
    const float mk = h * h * 0.25f - hh;
    gk = uni ? mk : -mk;    // the outer sign of -m(.)
  }
  const float mb = 1.0f - ma;
  gd = ma;                  // outer sign times a's sign: +1 for every operator
  gv = sub ? -mb : mb;      // outer sign times b's sign
}

// box_core's partials by q = |v| - b: the outside length's o_j / len and the
// inside maximum's one-hot (max(qx, max(qy, qz)), passed on while it is <= 0)
__device__ __forceinline__ void box_partials(V3 w, float bx, float by, float bz, float (&G)[3]) {
  const float qx = fabsf(w.x) - bx, qy = fabsf(w.y) - by, qz = fabsf(w.z) - bz;
  const float ox = gmax(qx, 0.0f), oy = gmax(qy, 0.0f), oz = gmax(qz, 0.0f);
  const float il = grcp(fsqrt(ox * ox + oy * oy + oz * oz));
  const bool zy = qy < qz;            // the inner max took qz
  const float in = zy ? qz : qy;
  const bool ix = !(qx < in);         // the outer max kept qx
  const float m = ix ? qx : in;
  const float pass = (0.0f < m) ? 0.0f : 1.0f;   // min(m, 0) took m
  // beside a face one component is positive and o / len is that axis exactly;
  // o_j * (1 / len) would be 1 -+ an ulp, which a round box's dr = G0 + G1 + G2 - 1
  // turns from an exact 0 into noise
  const bool px = qx > 0.0f, py = qy > 0.0f, pz = qz > 0.0f;
  const bool face = (int)px + (int)py + (int)pz == 1;
  G[0] = (face ? (px ? 1.0f : 0.0f) : ox * il) + (ix ? pass : 0.0f);
  G[1] = (face ? (py ? 1.0f : 0.0f) : oy * il) + ((!ix && !zy) ? pass : 0.0f);
  G[2] = (face ? (pz ? 1.0f : 0.0f) : oz * il) + ((!ix && zy) ? pass : 0.0f);
}

// dv/dp (gp) and dv/d(public p[j]) (t[0..6]) of primitive `kind` at p; `q` is
// the prepared block (sdf_abi.cpp prepare_prims), and the chain rule through it
// is taken here: a round box's half - r, a capsule's b - a and dot(ba, ba).
template <class Q>
__device__ __forceinline__ void prim_partials(int kind, V3 p, const Q& q, V3& gp, float (&t)[7]) {
#pragma unroll
  for (int j = 0; j < 7; j++) t[j] = 0.0f;
  switch (kind) {
    case SDF_PRIM_SPHERE: {
      const V3 w = sub(p, mk(q[0], q[1], q[2]));
      gp = muls(w, grcp(length(w)));
      t[0] = -gp.x, t[1] = -gp.y, t[2] = -gp.z, t[3] = -1.0f;
      break;
    }
    case SDF_PRIM_PLANE: {
      gp = mk(q[0], q[1], q[2]);
      t[0] = p.x, t[1] = p.y, t[2] = p.z, t[3] = 1.0f;
      break;
    }
    case SDF_PRIM_BOX:
    case SDF_PRIM_ROUND_BOX: {
      const V3 w = sub(p, mk(q[0], q[1], q[2]));
      float G[3];
      box_partials(w, q[3], q[4], q[5], G);
      gp = mk(gsign(w.x) * G[0], gsign(w.y) * G[1], gsign(w.z) * G[2]);
      t[0] = -gp.x, t[1] = -gp.y, t[2] = -gp.z;
      t[3] = -G[0], t[4] = -G[1], t[5] = -G[2];
      // box_core(v, half - r) - r: dr = -(-G0 - G1 - G2) - 1
      if (kind == SDF_PRIM_ROUND_BOX) t[6] = G[0] + G[1] + G[2] - 1.0f;
      break;
    }
    case SDF_PRIM_TORUS: {
      const V3 w = sub(p, mk(q[0], q[1], q[2]));
      const float lxz = fsqrt(w.x * w.x + w.z * w.z);
      const float qx = lxz - q[3];
      const float il = grcp(fsqrt(qx * qx + w.y * w.y));
      const float gq = qx * il;                 // dv/dqx
      const float r = gq * grcp(lxz);
      gp = mk(w.x * r, w.y * il, w.z * r);
      t[0] = -gp.x, t[1] = -gp.y, t[2] = -gp.z, t[3] = -gq, t[4] = -1.0f;
      break;
    }
    case SDF_PRIM_CAPSULE: {
      const V3 pa = sub(p, mk(q[0], q[1], q[2]));
      const V3 ba = mk(q[3], q[4], q[5]);
      const float n = dot(pa, ba);
      const float h0 = DIVK(n, q[7], q[8]);
      const float h = gclamp(h0, 0.0f, 1.0f);
      const V3 u = sub(pa, muls(ba, h));
      const V3 gu = muls(u, grcp(length(u)));   // dv/du
      // clamp = min(max(h0, 0), 1): max keeps h0 unless h0 < 0, min unless 1 < h0
      const float gh = (h0 < 0.0f || 1.0f < h0) ? 0.0f : -dot(ba, gu);
      const float gn = DIVK(gh, q[7], q[8]);    // dv/d dot(pa, ba)
      const float gbb = -(gn * h0);             // dv/d dot(ba, ba)
      gp = add(gu, muls(ba, gn));
      const V3 gba = add(add(muls(gu, -h), muls(pa, gn)), muls(ba, 2.0f * gbb));
      t[0] = -gp.x - gba.x, t[1] = -gp.y - gba.y, t[2] = -gp.z - gba.z;
      t[3] = gba.x, t[4] = gba.y, t[5] = gba.z, t[6] = -1.0f;
      break;
    }
    default: {   // SDF_PRIM_CYLINDER
      const V3 w = sub(p, mk(q[0], q[1], q[2]));
      const float lxz = fsqrt(w.x * w.x + w.z * w.z);
      const float dx = lxz - q[3], dy = fabsf(w.y) - q[4];
      const bool my = dx < dy;                  // max(dx, dy) took dy
      const float m = my ? dy : dx;
      const float pass = (0.0f < m) ? 0.0f : 1.0f;
      const float ox = gmax(dx, 0.0f), oy = gmax(dy, 0.0f);
      const float il = grcp(fsqrt(ox * ox + oy * oy));
      const float gx = ox * il + (my ? 0.0f : pass);
      const float gy = oy * il + (my ? pass : 0.0f);
      const float r = gx * grcp(lxz);
      gp = mk(w.x * r, gsign(w.y) * gy, w.z * r);
      t[0] = -gp.x, t[1] = -gp.y, t[2] = -gp.z, t[3] = -gx, t[4] = -gy;
      break;
    }
  }
}

// Eight sums across the wave at once: on return every lane holds the sum over
// the 64 lanes of t[lane & 7].  Three halving stages (xor 1, 2, 4) in which a lane
// keeps the half of its values its lane bit selects and adds the partner's
// copies of them -- 4 + 2 + 1 additions instead of 8 per stage -- then xor 8 and 16
// on the one value left (ds_swizzle) and xor 32 (ds_bpermute).  Partners add the
// same two numbers, and IEEE addition is commutative: the lanes of a term agree
// to the bit, and the order is fixed.
__device__ __forceinline__ float xor_add(float keep, float send, int j, int lane) {
  const uint32_t b = __float_as_uint(send);
  uint32_t r;
  switch (j) {
    case 1: r = xor_partner<1>(b); break;
    case 2: r = xor_partner<2>(b); break;
    case 4: r = xor_partner<4>(b); break;
    case 8: r = xor_partner<8>(b); break;
    case 16: r = xor_partner<16>(b); break;
    default: r = (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, (int)b); break;
  }
  return keep + __uint_as_float(r);
}
__device__ __forceinline__ float wave_sum8(const float (&t)[8], int lane) {
  const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0, b2 = (lane & 4) != 0;
  float u[4], w[2];
#pragma unroll
  for (int c = 0; c < 4; c++)
    u[c] = xor_add(b0 ? t[2 * c + 1] : t[2 * c], b0 ? t[2 * c] : t[2 * c + 1], 1, lane);
#pragma unroll
  for (int c = 0; c < 2; c++)
    w[c] = xor_add(b1 ? u[2 * c + 1] : u[2 * c], b1 ? u[2 * c] : u[2 * c + 1], 2, lane);
  float x = xor_add(b2 ? w[1] : w[0], b2 ? w[0] : w[1], 4, lane);
  x = xor_add(x, x, 8, lane);
  x = xor_add(x, x, 16, lane);
  return xor_add(x, x, 32, lane);
}

// One point of the gradient, in two halves that sample_grad and the sharp mesh
// kernel (mesh_kernel.inc) share.  fv / fd are the lane's own columns, rows
// STRIDE floats apart.
//
// The forward fold at p: GenericScene::eval's loop; with `park` it leaves v_j in
// fv[j STRIDE] and d_(j-1) in fd[j STRIDE].
template <int STRIDE>
__device__ __forceinline__ float grad_fold(KA& A, V3 p, bool park, float* fv, float* fd) {
  const int count = A.prim_count;
  float d = INFINITY;
#pragma unroll 1
  for (int j = 0; j < count; j++) {
    const KARG sdf_primitive& pr = A.prims[j];
    KF q = pr.p;
    const float v = prim_sdf(pr.kind, p, q);
    if (park) {
      fv[j * STRIDE] = v;
      fd[j * STRIDE] = d;
    }
    d = combine(pr.op, d, v, SMIN_K(pr), SMIN_IK(pr), SMIN_SC(pr), SMIN_KSC(pr));
  }
  return d;
}
// The backward sweep over what grad_fold parked, from the adjoint g of the
// scene's value: df/dp times g.  terms(j, av, ak, t) sees primitive j's adjoints
// and prim_partials' parameter terms (the parameter sums of sample_grad).  The
// skip of a primitive no lane needs is a ballot: every lane of the wave is here.
template <int STRIDE, class Terms>
__device__ __forceinline__ V3 grad_sweep(KA& A, V3 p, float g, const float* fv, const float* fd,
                                         Terms&& terms) {
  V3 gp = mk(0.0f, 0.0f, 0.0f);
#pragma unroll 1
  for (int j = A.prim_count - 1; j >= 0; j--) {
    const KARG sdf_primitive& pr = A.prims[j];
    KF q = pr.p;
    float gd, gv, gk;
    fold_partials(pr.op, fd[j * STRIDE], fv[j * STRIDE], SMIN_K(pr), SMIN_IK(pr), gd, gv, gk);
    const float av = g * gv;   // the adjoint of v_j
    const float ak = g * gk;   // this lane's term of the sum for k
    g = g * gd;
    if (__builtin_amdgcn_ballot_w64(av != 0.0f || ak != 0.0f) == 0) continue;
    V3 vp;
    float t[7];
    prim_partials(pr.kind, p, q, vp, t);
    gp = add(gp, muls(vp, av));
    terms(j, av, ak, t);
  }
  return gp;
}

#ifndef __HIPCC_RTC__   // the run-time specialiser takes the functions above alone
template <bool PRIMS>
__global__ __launch_bounds__(kGradBlock) void sample_grad(GradArgs args) {
  (void)args;
  const KARG GradArgs& G = *(const KARG GradArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  KA& A = G.a;
  // column tid of fv / fd: the primitives' values and the running distance
  // before each (LDS bank = tid mod 32: conflict-free)
  __shared__ float fv[SDF_MAX_PRIMS * kGradBlock];
  __shared__ float fd[SDF_MAX_PRIMS * kGradBlock];
  __shared__ double acc[PRIMS ? kGradWaves * kGradSlots : 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  if constexpr (PRIMS) {
#pragma unroll
    for (int j = 0; j < kGradSlots / 64; j++) acc[wave * kGradSlots + j * 64 + lane] = 0.0;
  }
  const bool backward = PRIMS || G.grad_points;
  const long long stride = (long long)gridDim.x * kGradBlock;
  // a wave runs while its first lane has a point, so every trip count is
  // wave-uniform; its lanes beyond n carry the last point with a zero adjoint
  // and store nothing
#pragma unroll 1
  for (long long base = (long long)blockIdx.x * kGradBlock + wave * 64; base < G.n; base += stride) {
    const long long i = base + lane;
    const bool live = i < G.n;
    const long long ii = live ? i : G.n - 1;
    const float* const o = G.points + 3 * ii;
    const V3 p = mk(o[0], o[1], o[2]);
    const float d = grad_fold<kGradBlock>(A, p, backward, fv + tid, fd + tid);
    if (G.dist && live) G.dist[i] = d;
    if (!backward) continue;
    float g = 0.0f;
    if (live) g = G.upstream ? G.upstream[i] : 1.0f;
    const V3 gp = grad_sweep<kGradBlock>(
        A, p, g, fv + tid, fd + tid, [&](int j, float av, float ak, const float (&t)[7]) {
          if constexpr (PRIMS) {
            // term 0 is k's (slot 2), term 1 + c is p[c]'s (slot 4 + c); lane l < 8 ends
            // up with the wave's sum of term l
            float t8[8];
            t8[0] = ak;
#pragma unroll
            for (int c = 0; c < 7; c++) t8[c + 1] = av * t[c];
            const float mine = wave_sum8(t8, lane);
            if (lane < 8) acc[wave * kGradSlots + j * 16 + (lane == 0 ? 2 : 3 + lane)] += (double)mine;
          } else {
            (void)j, (void)av, (void)ak, (void)t;
          }
        });
    if (G.grad_points && live) {
      float* const w = G.grad_points + 3 * i;
      w[0] = gp.x;
      w[1] = gp.y;
      w[2] = gp.z;
    }
  }
  if constexpr (PRIMS) {
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kGradWaves; w++) s += acc[w * kGradSlots + tid];
    G.rows[(size_t)blockIdx.x * kGradSlots + tid] = (float)s;
  }
}

// grad_prims[slot] = the fp64 sum of the workspace rows' slot in index order,
// rounded once: 4 segments of consecutive rows side by side, then the segments
// in order.  One workgroup of 4 x kGradSlots threads.
__global__ __launch_bounds__(4 * kGradSlots) void grad_reduce(const float* rows, int nrows,
                                                              float* out) {
  __shared__ double part[4 * kGradSlots];
  const int slot = threadIdx.x % kGradSlots, seg = threadIdx.x / kGradSlots;
  const int per = (nrows + 3) / 4;
  const int r0 = seg * per, r1 = min(nrows, r0 + per);
  // eight independent accumulators over interleaved rows keep eight loads in
  // flight; the order is as fixed as a single one's
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int r = r0;
  for (; r + 8 <= r1; r += 8) {
#pragma unroll
    for (int u = 0; u < 8; u++) a[u] += (double)rows[(size_t)(r + u) * kGradSlots + slot];
  }
  for (; r < r1; r++) a[0] += (double)rows[(size_t)r * kGradSlots + slot];
  const double s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  part[seg * kGradSlots + slot] = s;
  __syncthreads();
  if (seg == 0)
    out[slot] = (float)(((part[slot] + part[kGradSlots + slot]) + part[2 * kGradSlots + slot]) +
                        part[3 * kGradSlots + slot]);
}
#endif  // !__HIPCC_RTC__
