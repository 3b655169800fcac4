// pt_ploc.hip -- a BVH built on the device by parallel locally-ordered clustering (mi3pt_device_build_bvh_ex, method 1).
//
// Meister and Bittner, "Parallel Locally-Ordered Clustering for Bounding Volume Hierarchy Construction" (TVCG 2018): the triangles in
// Morton order are clusters; every iteration each cluster looks `radius` positions to either side for the neighbour whose union with it
// has the least area, mutual choices merge, the survivors close ranks.  Bottom-up, so the trees are of the SAH class --
// unlike the linear builder's (pt_lbvh.hip), whose leaf, key and sort step this one calls (pt_lbvh.h).
//
// THE LAW is in include/mi3pt.h (mi3pt_device_build_bvh_ex) and restated in tests/ploc_reference.py; the output is a function of the
// triangle records, the radius and the search budget alone.  What is free here, and does not show in the output:
//   - temporary node ids: leaf p (sorted position) is id p, an internal node takes n + atomicAdd(counter).  Only the topology reaches the
//     output, because the final numbering is the pre-order one;
//   - the cut into kernels.  Per iteration: k_ploc_search (or k_ploc_pairing once the search budget is used up) writes nn[]; an exclusive
//     prefix sum of the keep flags (hipCUB, the flags computed on the fly from nn[]) gives every survivor its new position; k_ploc_merge
//     forms the merged clusters and moves all survivors into the other buffer, and its last thread writes the new cluster count to pinned
//     host memory.  The host reads those 4 bytes after a stream synchronise and drives the next iteration: no thread ever waits for another.
//   - k_ploc_emit: one thread per node sums, up its path to the root, 1 for a left child and 2 x leaves(left sibling) for a right child:
//     its pre-order index.
//
// k_ploc_search stages its block's PLOC_BLOCK clusters plus a halo of `radius` on each side in LDS once, structure-of-arrays fp32: for a
// candidate offset the lanes of a wave read consecutive words of one array (no bank conflict); read from global memory the window would
// be fetched 2 x radius times.  6 x (256 + 128) x 4 B = 9 KiB of LDS.
#include "pt_internal.h"
#include "pt_lbvh.h"
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstdint>
#include <string>

namespace pt {

constexpr int PLOC_BLOCK = MI3PT_PLOC_SEARCH_BLOCK;          // include/mi3pt.h: the tests cross its edges
constexpr int PLOC_MAX_RADIUS = 64;
static_assert(PLOC_BLOCK == 256, "k_ploc_search's launch bounds and LDS size");

// clusters, structure of arrays: c[0..2] the minima, c[3..5] the maxima, id the subtree
struct Clusters { float *c[6]; int *id; };

// d of the law for the boxes a (lower position) and b: the half area of the union, a NaN as +inf
__device__ __forceinline__ float ploc_distance(const float a[6], const float b[6])
{
    const float ex = fmaxf(a[3], b[3]) - fminf(a[0], b[0]);
    const float ey = fmaxf(a[4], b[4]) - fminf(a[1], b[1]);
    const float ez = fmaxf(a[5], b[5]) - fminf(a[2], b[2]);
    const float area = (ex * ey + ey * ez) + ez * ex;
    return area == area ? area : __int_as_float(0x7f800000);
}

__global__ void __launch_bounds__(256) k_ploc_init(const uint32_t *__restrict__ order, int n, const Box *__restrict__ tri_box, Clusters cl,
                                                   int *__restrict__ leaves)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const Box b = tri_box[order[p]];
    for (int k = 0; k < 3; k++) { cl.c[k][p] = b.mn[k]; cl.c[3 + k][p] = b.mx[k]; }
    cl.id[p] = p;
    leaves[p] = 1;
}

// nn[i]: the position j != i, |i - j| <= radius, 0 <= j < C, with the least key (d, |i - j|, min(i, j) & 1, min(i, j))
__global__ void __launch_bounds__(PLOC_BLOCK) k_ploc_search(Clusters cl, int C, int radius, int *__restrict__ nn)
{
    __shared__ float s[6][PLOC_BLOCK + 2 * PLOC_MAX_RADIUS];
    const int base = blockIdx.x * PLOC_BLOCK - radius;                    // position of s[.][0]
    for (int t = threadIdx.x; t < PLOC_BLOCK + 2 * radius; t += PLOC_BLOCK) {
        const int p = base + t;
        if (p >= 0 && p < C)
            for (int k = 0; k < 6; k++) s[k][t] = cl.c[k][p];
    }
    __syncthreads();
    const int i = blockIdx.x * PLOC_BLOCK + threadIdx.x;
    if (i >= C) return;
    const int me = threadIdx.x + radius;
    float mine[6];
    for (int k = 0; k < 6; k++) mine[k] = s[k][me];
    float best_d = 0.0f;
    int best_k = 0, best_a = 0, best_j = -1;
    for (int k = 1; k <= radius; k++) {                                   // ascending: at equal d the smaller offset stays
        if (i - k >= 0) {                                                 // the pair (i - k, i)
            float other[6];
            for (int c = 0; c < 6; c++) other[c] = s[c][me - k];
            const float d = ploc_distance(other, mine);
            if (best_j < 0 || d < best_d) { best_d = d; best_k = k; best_a = i - k; best_j = i - k; }
        }
        if (i + k < C) {                                                  // the pair (i, i + k)
            float other[6];
            for (int c = 0; c < 6; c++) other[c] = s[c][me + k];
            const float d = ploc_distance(mine, other);
            const bool tie = d == best_d && k == best_k;                  // only with (i - k, i): then (a & 1, a) decides
            if (best_j < 0 || d < best_d || (tie && ((i & 1) < (best_a & 1) || ((i & 1) == (best_a & 1) && i < best_a)))) {
                best_d = d; best_k = k; best_a = i; best_j = i + k;
            }
        }
    }
    nn[i] = best_j;
}

// a forced iteration: nn[i] = i ^ 1 where that is a position, else none
__global__ void __launch_bounds__(256) k_ploc_pairing(int C, int *__restrict__ nn)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C) return;
    nn[i] = (i ^ 1) < C ? (i ^ 1) : -1;
}

// 1 unless position i is the upper one of a mutual pair
struct PlocKeep {
    const int *nn;
    __host__ __device__ int operator()(int i) const
    {
        const int j = nn[i];
        return (j >= 0 && j < i && nn[j] == i) ? 0 : 1;
    }
};

// per node id: parent and the node's distance from its parent in pre-order; per internal node (id - n): box and the leaves of its left child
struct PlocNodes { int *parent, *offset, *leaves, *left_leaves; Box *box; };

__global__ void __launch_bounds__(256) k_ploc_merge(Clusters from, Clusters to, int C, const int *__restrict__ nn, const int *__restrict__ pos,
                                                    int n, PlocNodes nd, int *__restrict__ next_id, int *__restrict__ count_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C) return;
    const int j = nn[i];
    const bool mutual = j >= 0 && nn[j] == i;
    const bool kept = !(mutual && j < i);
    if (i == C - 1) *count_out = pos[i] + (kept ? 1 : 0);
    if (!kept) return;
    const int dst = pos[i];
    if (!mutual) {
        for (int k = 0; k < 6; k++) to.c[k][dst] = from.c[k][i];
        to.id[dst] = from.id[i];
        return;
    }
    const int id = atomicAdd(next_id, 1), l = from.id[i], r = from.id[j];
    Box u;
    for (int k = 0; k < 3; k++) {
        u.mn[k] = fminf(from.c[k][i], from.c[k][j]);
        u.mx[k] = fmaxf(from.c[3 + k][i], from.c[3 + k][j]);
        to.c[k][dst] = u.mn[k];
        to.c[3 + k][dst] = u.mx[k];
    }
    to.id[dst] = id;
    const int ll = nd.leaves[l];
    nd.leaves[id] = ll + nd.leaves[r];
    nd.left_leaves[id - n] = ll;
    nd.box[id - n] = u;
    nd.parent[l] = id; nd.offset[l] = 1;
    nd.parent[r] = id; nd.offset[r] = 2 * ll;
}

// the 48-byte record of every node at its pre-order index; parent[] of the root is -1
__global__ void __launch_bounds__(256) k_ploc_emit(const uint32_t *__restrict__ order, int n, const Box *__restrict__ tri_box, PlocNodes nd,
                                                   uint8_t *__restrict__ out)
{
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= 2 * n - 1) return;
    int idx = 0;
    for (int x = node; nd.parent[x] >= 0; x = nd.parent[x]) idx += nd.offset[x];
    const bool leaf = node < n;
    const Box b = leaf ? tri_box[order[node]] : nd.box[node - n];
    float *f = reinterpret_cast<float *>(out + (size_t)idx * 48);
    int *w = reinterpret_cast<int *>(out + (size_t)idx * 48);
    f[0] = b.mn[0]; f[1] = b.mn[1]; f[2] = b.mn[2]; w[3] = 0;
    f[4] = b.mx[0]; f[5] = b.mx[1]; f[6] = b.mx[2];
    if (leaf) {
        w[7] = 1; w[8] = -1; w[9] = -1; w[10] = (int)order[node];
    } else {
        w[7] = 0; w[8] = idx + 1; w[9] = idx + 2 * nd.left_leaves[node - n]; w[10] = -1;
    }
    w[11] = 0;
}

#define PL_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); goto done; } } while (0)

// tris: device pointer to n 112-byte records; nodes_out: HOST buffer of (2n - 1) x 48 bytes.  radius 1 .. 64.
int ploc_build(const void *d_tris, size_t n, int radius, int max_search_iterations, void *nodes_out, float *build_ms,
               uint32_t *search_iterations, uint32_t *forced_iterations, hipStream_t stream, std::string &err)
{
    if (n == 0) { err = "no triangles"; return -1; }
    if (radius < 1 || radius > PLOC_MAX_RADIUS) { err = "radius out of range"; return -1; }
    if (n > (size_t)1 << 29) { err = "too many triangles"; return -1; }                 // 2n - 1 records, 2 x leaves in an int
    const int N = (int)n;
    const size_t nodes = 2 * n - 1;
    SortedLeaves lv;
    float *cbox = nullptr;                      // 2 buffers x 6 arrays x n
    int *cid = nullptr;                         // 2 x n
    int *nn = nullptr, *pos = nullptr, *next_id = nullptr, *h_count = nullptr, *d_count = nullptr;
    PlocNodes nd = { nullptr, nullptr, nullptr, nullptr, nullptr };
    uint8_t *d_out = nullptr;
    void *scan_tmp = nullptr;
    size_t scan_bytes = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    Clusters cl[2];
    int cur = 0, C = N;
    uint32_t searched = 0, forced = 0;
    float ms = 0.0f;
    hipcub::CountingInputIterator<int> counting(0);
    PL_TRY(hipMalloc((void **)&cbox, 2 * 6 * n * 4));
    PL_TRY(hipMalloc((void **)&cid, 2 * n * 4));
    PL_TRY(hipMalloc((void **)&nn, n * 4));
    PL_TRY(hipMalloc((void **)&pos, n * 4));
    PL_TRY(hipMalloc((void **)&next_id, 4));
    PL_TRY(hipMalloc((void **)&nd.parent, nodes * 4));
    PL_TRY(hipMalloc((void **)&nd.offset, nodes * 4));
    PL_TRY(hipMalloc((void **)&nd.leaves, nodes * 4));
    PL_TRY(hipMalloc((void **)&nd.left_leaves, n * 4));
    PL_TRY(hipMalloc((void **)&nd.box, n * sizeof(Box)));
    PL_TRY(hipMalloc((void **)&d_out, nodes * 48));
    PL_TRY(hipHostMalloc((void **)&h_count, 4, hipHostMallocDefault));
    PL_TRY(hipHostGetDevicePointer((void **)&d_count, h_count, 0));
    {
        hipcub::TransformInputIterator<int, PlocKeep, hipcub::CountingInputIterator<int>> keep(counting, PlocKeep{ nn });
        PL_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, keep, pos, N, stream));
    }
    PL_TRY(hipMalloc(&scan_tmp, scan_bytes ? scan_bytes : 16));
    PL_TRY(hipEventCreate(&e0));
    PL_TRY(hipEventCreate(&e1));
    PL_TRY(sorted_leaves_prepare(n, lv, stream));
    for (int b = 0; b < 2; b++) {
        for (int k = 0; k < 6; k++) cl[b].c[k] = cbox + ((size_t)b * 6 + (size_t)k) * n;
        cl[b].id = cid + (size_t)b * n;
    }
    PL_TRY(hipMemsetAsync(nd.parent, 0xff, nodes * 4, stream));
    PL_TRY(hipMemsetAsync(nd.offset, 0, nodes * 4, stream));
    PL_TRY(hipMemcpyAsync(next_id, &N, 4, hipMemcpyHostToDevice, stream));
    PL_TRY(hipEventRecord(e0, stream));
    PL_TRY(sorted_leaves_enqueue(d_tris, n, lv, stream));
    hipLaunchKernelGGL(k_ploc_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, lv.order, N, lv.tri_box, cl[0], nd.leaves);
    while (C > 1) {
        const unsigned blocks = (unsigned)((C + 255) / 256);
        if (searched < (uint32_t)max_search_iterations) {
            hipLaunchKernelGGL(k_ploc_search, dim3((unsigned)((C + PLOC_BLOCK - 1) / PLOC_BLOCK)), dim3(PLOC_BLOCK), 0, stream, cl[cur], C, radius, nn);
            searched++;
        } else {
            hipLaunchKernelGGL(k_ploc_pairing, dim3(blocks), dim3(256), 0, stream, C, nn);
            forced++;
        }
        hipcub::TransformInputIterator<int, PlocKeep, hipcub::CountingInputIterator<int>> keep(counting, PlocKeep{ nn });
        PL_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, keep, pos, C, stream));
        hipLaunchKernelGGL(k_ploc_merge, dim3(blocks), dim3(256), 0, stream, cl[cur], cl[cur ^ 1], C, nn, pos, N, nd, next_id, d_count);
        PL_TRY(hipGetLastError());
        PL_TRY(hipStreamSynchronize(stream));
        const int next = *(volatile int *)h_count;
        if (next < 1 || next >= C) { err = "the clustering made no progress"; goto done; }       // (the law's least pair is mutual: cannot happen)
        C = next;
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_ploc_emit, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, stream, lv.order, N, lv.tri_box, nd, d_out);
    PL_TRY(hipGetLastError());
    PL_TRY(hipEventRecord(e1, stream));
    PL_TRY(hipMemcpyAsync(nodes_out, d_out, nodes * 48, hipMemcpyDeviceToHost, stream));
    PL_TRY(hipStreamSynchronize(stream));
    PL_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (build_ms) *build_ms = ms;
    if (search_iterations) *search_iterations = searched;
    if (forced_iterations) *forced_iterations = forced;
done:
    if (!err.empty()) (void)hipStreamSynchronize(stream);                  // nothing queued may still use what is freed below
    sorted_leaves_free(lv);
    for (void *p : { (void *)cbox, (void *)cid, (void *)nn, (void *)pos, (void *)next_id, (void *)nd.parent, (void *)nd.offset, (void *)nd.leaves,
                     (void *)nd.left_leaves, (void *)nd.box, (void *)d_out, scan_tmp })
        if (p) (void)hipFree(p);
    if (h_count) (void)hipHostFree(h_count);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return err.empty() ? 0 : -1;
}

}  // namespace pt
