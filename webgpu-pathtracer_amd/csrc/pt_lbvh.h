// pt_lbvh.h -- the first half of the linear builder (pt_lbvh.hip), shared with the clustering builder (pt_ploc.hip): per triangle the
// NaN-ignoring box and centroid, the 63-bit Morton keys, a stable radix sort.  One implementation, so that both builders see the same
// leaves in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace pt {

struct Box { float mn[3], mx[3]; };

struct SortedLeaves {
    Box *tri_box = nullptr;                               // per triangle, in triangle order
    unsigned long long *keys_sorted = nullptr;            // ascending
    uint32_t *order = nullptr;                            // the triangle at every sorted position
    // temporaries of the step
    float *centroid = nullptr;
    int *bounds = nullptr;
    unsigned long long *keys = nullptr;
    uint32_t *vals = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
};
// allocates for n triangles and queues the initial values on `stream`; on an error the caller frees what was allocated
hipError_t sorted_leaves_prepare(size_t n, SortedLeaves &s, hipStream_t stream);
// queues the three steps on `stream`: tri_box, keys_sorted and order are ready when it has run
hipError_t sorted_leaves_enqueue(const void *d_tris, size_t n, SortedLeaves &s, hipStream_t stream);
void sorted_leaves_free(SortedLeaves &s);

}  // namespace pt
