// mesh.hip -- the scan between sdf_mesh_count and sdf_mesh_emit (sdf_abi.h
// "Meshes"): the bricks' vertex and triangle counts become each brick's
// offsets, and their totals the call's `counts`.  Three launches over chunks
// of kMeshScanChunk bricks: the chunks' sums, one workgroup's exclusive scan
// of those sums (it also writes the totals), the offsets inside each chunk.
// Everything is summed in a fixed order in 64-bit integers: no atomics, the
// same offsets on every run.
#include <hip/hip_runtime.h>

#include "host_api.h"   // this unit's launcher prototypes (and kernel_args.h)

namespace sdf {
namespace {

struct Sum3 {
  long long v, t, e;   // vertices, triangles, evaluated bricks
};
__device__ __forceinline__ Sum3 add3(Sum3 a, Sum3 b) { return Sum3{a.v + b.v, a.t + b.t, a.e + b.e}; }
__device__ __forceinline__ Sum3 of_brick(const MeshBrick& b) {
  return Sum3{(long long)(b.nv & ~kMeshEvaluated), (long long)b.nt, (long long)(b.nv >> 31)};
}

// Exclusive scan of one value per thread over the workgroup's kMeshScanChunk
// threads (16 waves); `total` receives the workgroup's sum.
__device__ __forceinline__ Sum3 block_exscan(Sum3 x, Sum3& total) {
  __shared__ Sum3 wsum[kMeshScanChunk / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Sum3 inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Sum3 y{__shfl_up(inc.v, d), __shfl_up(inc.t, d), __shfl_up(inc.e, d)};
    if (lane >= d) inc = add3(inc, y);
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  Sum3 base{0, 0, 0}, tot{0, 0, 0};
  for (int k = 0; k < kMeshScanChunk / 64; k++) {
    if (k < wave) base = add3(base, wsum[k]);
    tot = add3(tot, wsum[k]);
  }
  __syncthreads();   // wsum is written again by the next call
  total = tot;
  return Sum3{base.v + inc.v - x.v, base.t + inc.t - x.t, base.e + inc.e - x.e};
}

__global__ __launch_bounds__(kMeshScanChunk) void mesh_scan_sums(const MeshBrick* bricks,
                                                                 long long n, long long* sums) {
  const long long i = (long long)blockIdx.x * kMeshScanChunk + threadIdx.x;
  Sum3 total;
  (void)block_exscan(i < n ? of_brick(bricks[i]) : Sum3{0, 0, 0}, total);
  if (threadIdx.x == 0) {
    long long* const o = sums + 3 * (long long)blockIdx.x;
    o[0] = total.v;
    o[1] = total.t;
    o[2] = total.e;
  }
}

// one workgroup: the chunk sums become the sums of the chunks before each
__global__ __launch_bounds__(kMeshScanChunk) void mesh_scan_top(long long* sums, long long chunks,
                                                                long long nbricks,
                                                                long long* counts) {
  Sum3 carry{0, 0, 0};
  for (long long base = 0; base < chunks; base += kMeshScanChunk) {
    const long long i = base + threadIdx.x;
    Sum3 x{0, 0, 0};
    if (i < chunks) x = Sum3{sums[3 * i], sums[3 * i + 1], sums[3 * i + 2]};
    Sum3 total;
    const Sum3 ex = add3(carry, block_exscan(x, total));
    if (i < chunks) {
      sums[3 * i] = ex.v;
      sums[3 * i + 1] = ex.t;
      sums[3 * i + 2] = ex.e;
    }
    carry = add3(carry, total);
  }
  if (threadIdx.x == 0) {
    counts[0] = carry.v;
    counts[1] = carry.t;
    counts[2] = carry.e;
    counts[3] = nbricks;
  }
}

__global__ __launch_bounds__(kMeshScanChunk) void mesh_scan_offsets(const MeshBrick* bricks,
                                                                    long long n,
                                                                    const long long* sums,
                                                                    MeshOffset* offsets) {
  const long long i = (long long)blockIdx.x * kMeshScanChunk + threadIdx.x;
  Sum3 total;
  const Sum3 ex = block_exscan(i < n ? of_brick(bricks[i]) : Sum3{0, 0, 0}, total);
  if (i < n) {
    const long long* const b = sums + 3 * (long long)blockIdx.x;
    offsets[i] = MeshOffset{b[0] + ex.v, b[1] + ex.t};
  }
}

}  // namespace

int launch_mesh_scan(unsigned char* ws, long long nbricks, long long* counts, void* stream) {
  if (!ws || !counts || nbricks <= 0) return (int)hipErrorInvalidValue;
  const MeshLayout L(nbricks);
  const long long chunks = (nbricks + kMeshScanChunk - 1) / kMeshScanChunk;
  if (chunks > 0x7fffffffll) return (int)hipErrorInvalidValue;
  const MeshBrick* const bricks = (const MeshBrick*)(ws + L.brick);
  long long* const sums = (long long*)(ws + L.sums);
  MeshOffset* const offsets = (MeshOffset*)(ws + L.offset);
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(kMeshScanChunk), grid((unsigned)chunks);
  (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
  hipLaunchKernelGGL(mesh_scan_sums, grid, block, 0, s, bricks, nbricks, sums);
  hipLaunchKernelGGL(mesh_scan_top, dim3(1), block, 0, s, sums, chunks, nbricks, counts);
  hipLaunchKernelGGL(mesh_scan_offsets, grid, block, 0, s, bricks, nbricks, sums, offsets);
  return (int)hipGetLastError();
}

}  // namespace sdf
