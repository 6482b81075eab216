// mesh.hip -- the scan between sdf_mesh_count and sdf_mesh_emit (sdf_abi.h
// "Meshes"): the bricks' vertex and triangle counts become each brick's
// offsets, and their totals the call's `counts`.  Three launches over chunks
// of kMeshScanChunk bricks: the chunks' sums, one workgroup's exclusive scan
// of those sums (it also writes the totals), the offsets inside each chunk.
// Everything is summed in a fixed order in 64-bit integers: no atomics, the
// same offsets on every run.
//
// And the second half of sdf_measure ("Measures"): measure_reduce combines the
// records the measure kernel's workgroups wrote (kernel_args.h MeasureArgs) into
// the call's `moments` and `counts` -- sums, and min / max for lo / hi.  Integers:
// any order gives the same bits.
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

// Workgroup g < rows: row g of every record into moments[16 g ..]; workgroup
// `rows`: the records' tails into counts.  Thread = (segment, slot): 64
// segments of interleaved records, four independent loads in flight per thread
// (a thread's loads are otherwise one dependent chain: with 16 segments over
// 4,096 records the combination took longer than the measure kernel at 128^3
// cells), combined through LDS.
constexpr int kMeasureReduceSegs = 64;
constexpr int kMeasureReduceUnroll = 4;
__device__ __forceinline__ long long measure_reduce_op(bool lo, bool hi, long long v, long long x) {
  return lo ? (x < v ? x : v) : hi ? (x > v ? x : v) : v + x;
}
__global__ __launch_bounds__(kMeasureReduceSegs * SDF_MEASURE_SLOTS) void measure_reduce(
    const long long* ws, int nblocks, int rows, long long nbricks, long long* moments,
    long long* counts) {
  __shared__ long long part[kMeasureReduceSegs * SDF_MEASURE_SLOTS];
  const int slot = threadIdx.x % SDF_MEASURE_SLOTS, seg = threadIdx.x / SDF_MEASURE_SLOTS;
  const int g = blockIdx.x;
  const bool tail = g == rows;
  const int rec = measure_record(rows);
  const bool lo = !tail && slot >= kMeasureLo && slot < kMeasureHi;
  const bool hi = !tail && slot >= kMeasureHi;
  const bool live = !tail || slot < kMeasureTail;
  const long long big = 0x7fffffffffffffffll;
  const long long unit = lo ? big : hi ? -big : 0;
  long long v = unit;
  if (live) {
    const long long* const p = ws + (size_t)g * SDF_MEASURE_SLOTS + slot;
    long long a[kMeasureReduceUnroll];
#pragma unroll
    for (int u = 0; u < kMeasureReduceUnroll; u++) a[u] = unit;
    for (int b = seg; b < nblocks; b += kMeasureReduceUnroll * kMeasureReduceSegs) {
#pragma unroll
      for (int u = 0; u < kMeasureReduceUnroll; u++) {
        const int bb = b + u * kMeasureReduceSegs;
        if (bb < nblocks) a[u] = measure_reduce_op(lo, hi, a[u], p[(size_t)bb * rec]);
      }
    }
#pragma unroll
    for (int u = 0; u < kMeasureReduceUnroll; u++) v = measure_reduce_op(lo, hi, v, a[u]);
  }
  part[threadIdx.x] = v;
  __syncthreads();
  if (seg != 0 || !live) return;
  for (int k = 1; k < kMeasureReduceSegs; k++)
    v = measure_reduce_op(lo, hi, v, part[k * SDF_MEASURE_SLOTS + slot]);
  if (!tail) moments[(size_t)g * SDF_MEASURE_SLOTS + slot] = v;
  else counts[slot] = slot < 2 ? v : slot == 2 ? nbricks : 0;
}

}  // namespace

int launch_measure_reduce(const long long* ws, int nblocks, int rows, long long nbricks,
                          long long* moments, long long* counts, void* stream) {
  if (!ws || !moments || !counts || nblocks <= 0 || nblocks > kMeasureMaxBlocks ||
      (rows != 1 && rows != SDF_MEASURE_ROWS))
    return (int)hipErrorInvalidValue;
  (void)hipGetLastError();  // a stale error of an earlier call is not this launch's
  hipLaunchKernelGGL(measure_reduce, dim3(rows + 1), dim3(kMeasureReduceSegs * SDF_MEASURE_SLOTS), 0,
                     (hipStream_t)stream, ws, nblocks, rows, nbricks, moments, counts);
  return (int)hipGetLastError();
}

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
