// pt_refit.hip -- re-fit the boxes of an uploaded BVH to the triangle records as they stand (mi3pt_device_refit_bvh).
//
// NOT a build: the topology -- words 7 .. 10 of every 48-byte record (raytrace.wgsl:51-64) -- stays, only the boxes follow the
// vertices.  The reference's boxes are exact (a leaf box is Box3.setFromPoints(a, b, c), an internal box the union of its inputs,
// raytrace.ts:546-550, 581-584) and rounding to fp32 is monotone, so a bottom-up min / max over the fp32 triangle records gives the
// boxes the reference's build would give THIS topology, bit for bit: re-fitting an unchanged scene returns the uploaded bytes.
//
// The law, per component (Math.min / Math.max on zeros; a NaN y is dropped, a NaN x is kept):
//   lo(x, y) = (y < x || (y == x && signbit(y))) ? y : x        hi(x, y) = (y > x || (y == x && !signbit(y))) ? y : x
//   leaf:      min = lo(lo(a, b), c), max = hi(hi(a, b), c)     a, b, c: the three positions of record `triangleIndex`
//   internal:  min = lo(min(left), min(right)), max = hi(max(left), max(right))     always left then right
// Words 3 and 7 .. 11 are carried bit for bit.
//
// One thread per node.  k_refit_parents: over a table of -1, every internal node names itself as the parent of its two children (a proper
// tree whose every record the root reaches: each node but the root is written exactly once, the root keeps its -1).  k_refit_fit: every leaf writes its box and climbs;
// at a parent the first child to arrive leaves, the second forms the union of (left, right) and climbs on -- the scheme of
// k_lbvh_fit (pt_lbvh.hip).  No thread waits for another: no spin, no retry.  A parent's index is below its child's
// (mi3pt_upload_bvh refuses anything else), so every climb ends at node 0 after fewer than 64 steps.
// Hand-off between the two children of a node: plain stores of the box, an agent-scope release (__threadfence) with the stores
// drained behind it, the arrival counter's atomic add; the second arriver fences again (acquire: its CU's L1 drops stale lines) and
// reads both children with plain vector loads.  The records being fitted are never read through a const __restrict__ pointer (scalar
// path).  Everything that is NOT a box -- the leaf flag, the child and triangle indices, the carried words 3 and 7 -- is read from the
// uploaded records, which no kernel of the call writes: the only words of the copy a thread reads are boxes handed to it as above.
// The range checks in both kernels cannot fire: mi3pt_upload_bvh has refused a child outside (parent, n), mi3pt_device_refit_bvh a
// tree that is not proper (depth under 64, both children present), a record the root does not reach and a leaf whose triangle does not
// exist.  They stay because a kernel that trusts words it read from memory for an address can take a machine down; were one to fire,
// the boxes above it would keep their uploaded values.
#include "pt_internal.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

namespace pt {

__device__ __forceinline__ bool refit_neg(float f) { return (__float_as_uint(f) >> 31) != 0u; }
__device__ __forceinline__ float refit_lo(float x, float y) { return (y < x || (y == x && refit_neg(y))) ? y : x; }
__device__ __forceinline__ float refit_hi(float x, float y) { return (y > x || (y == x && !refit_neg(y))) ? y : x; }

__global__ void __launch_bounds__(256) k_refit_parents(const int4 *__restrict__ nodes, uint32_t n, int *__restrict__ parent)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int is_leaf = nodes[(size_t)i * 3 + 1].w;
    if (is_leaf == 1) return;
    const int4 w = nodes[(size_t)i * 3 + 2];        // left, right, triangleIndex, pad
    // (both inside (i, n) by the upload's validation and tree_proper: see the note on range checks above)
    if ((uint32_t)w.x > i && (uint32_t)w.x < n) parent[w.x] = (int)i;
    if ((uint32_t)w.y > i && (uint32_t)w.y < n) parent[w.y] = (int)i;
}

// nodes: the uploaded records (read only); out: their device copy, whose boxes are re-fitted in place
__global__ void __launch_bounds__(256) k_refit_fit(const float4 *__restrict__ tris, uint32_t ntris, const float4 *__restrict__ nodes, float4 *out,
                                                   uint32_t n, const int *__restrict__ parent, int *arrived)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 r1 = nodes[(size_t)i * 3 + 1];
    if (__float_as_int(r1.w) != 1) return;          // an internal node: its second child writes it
    float4 r0 = nodes[(size_t)i * 3 + 0];
    const uint32_t ti = (uint32_t)__float_as_int(nodes[(size_t)i * 3 + 2].z);
    if (ti >= ntris) return;                         // (cannot fire: max_tri_ref < ntris is checked on the host)
    const float4 a = tris[(size_t)ti * 7 + 0], b = tris[(size_t)ti * 7 + 1], c = tris[(size_t)ti * 7 + 2];
    r0.x = refit_lo(refit_lo(a.x, b.x), c.x); r0.y = refit_lo(refit_lo(a.y, b.y), c.y); r0.z = refit_lo(refit_lo(a.z, b.z), c.z);
    r1.x = refit_hi(refit_hi(a.x, b.x), c.x); r1.y = refit_hi(refit_hi(a.y, b.y), c.y); r1.z = refit_hi(refit_hi(a.z, b.z), c.z);
    out[(size_t)i * 3 + 0] = r0;
    out[(size_t)i * 3 + 1] = r1;
    int p = parent[i];
    for (int step = 0; p >= 0 && step < 64; step++) {           // (the step bound cannot bind: a proper tree is under 64 deep)
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the box is out before the arrival is counted
        if (atomicAdd(arrived + p, 1) == 0) return;             // the sibling will finish this node
        __threadfence();
        const int4 w = reinterpret_cast<const int4 *>(nodes)[(size_t)p * 3 + 2];
        if ((uint32_t)w.x >= n || (uint32_t)w.y >= n) return;      // (cannot fire: see the note on range checks above)
        const float4 l0 = out[(size_t)w.x * 3 + 0], l1 = out[(size_t)w.x * 3 + 1];
        const float4 q0 = out[(size_t)w.y * 3 + 0], q1 = out[(size_t)w.y * 3 + 1];
        float4 p0 = nodes[(size_t)p * 3 + 0], p1 = nodes[(size_t)p * 3 + 1];      // (for words 3 and 7)
        p0.x = refit_lo(l0.x, q0.x); p0.y = refit_lo(l0.y, q0.y); p0.z = refit_lo(l0.z, q0.z);
        p1.x = refit_hi(l1.x, q1.x); p1.y = refit_hi(l1.y, q1.y); p1.z = refit_hi(l1.z, q1.z);
        out[(size_t)p * 3 + 0] = p0;
        out[(size_t)p * 3 + 1] = p1;
        p = parent[p];
    }
}

#define RF_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); goto done; } } while (0)

// d_tris: ntris 112-byte records, d_nodes: n 48-byte records, both on the device and left as they are; nodes_out: HOST buffer of n * 48 bytes
int refit_bvh(const void *d_tris, size_t ntris, const void *d_nodes, size_t n, void *nodes_out, float *refit_ms, hipStream_t stream, std::string &err)
{
    if (n == 0 || ntris == 0) { err = "no scene"; return -1; }
    uint8_t *work = nullptr;                 // n x 48 records | n x 4 parents | n x 4 arrival counters
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    float ms = 0.0f;
    RF_TRY(hipMalloc((void **)&work, n * (48 + 4 + 4)));
    {
        float4 *out = reinterpret_cast<float4 *>(work);
        int *parent = reinterpret_cast<int *>(work + n * 48), *arrived = parent + n;
        RF_TRY(hipEventCreate(&e0));
        RF_TRY(hipEventCreate(&e1));
        RF_TRY(hipEventRecord(e0, stream));
        RF_TRY(hipMemcpyAsync(out, d_nodes, n * 48, hipMemcpyDeviceToDevice, stream));
        RF_TRY(hipMemsetAsync(parent, 0xff, n * 4, stream));        // (-1: a slot no internal node writes ends a climb, it cannot misdirect one)
        hipLaunchKernelGGL(k_refit_parents, dim3(blocks), dim3(256), 0, stream, static_cast<const int4 *>(d_nodes), (uint32_t)n, parent);
        RF_TRY(hipMemsetAsync(arrived, 0, n * 4, stream));
        hipLaunchKernelGGL(k_refit_fit, dim3(blocks), dim3(256), 0, stream, static_cast<const float4 *>(d_tris), (uint32_t)ntris,
                           static_cast<const float4 *>(d_nodes), out, (uint32_t)n, parent, arrived);
        RF_TRY(hipGetLastError());
        RF_TRY(hipEventRecord(e1, stream));
        RF_TRY(hipMemcpyAsync(nodes_out, out, n * 48, hipMemcpyDeviceToHost, stream));
        RF_TRY(hipStreamSynchronize(stream));
        RF_TRY(hipEventElapsedTime(&ms, e0, e1));
        if (refit_ms) *refit_ms = ms;
    }
done:
    if (work) (void)hipFree(work);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return err.empty() ? 0 : -1;
}

}  // namespace pt
