// cv2.inpaint(INPAINT_TELEA) -- cluster bookkeeping for the cluster-parallel march (shape_ftp.py:652-666).
//
// Telea's march is ordered by a stable priority queue (T, push sequence), but hole pixels farther apart
// than their (2*range+1)^2 neighbourhoods plus the outside T ring can never see each other: restricted to
// such an independent CLUSTER of hole pixels the queue pops in exactly the same relative order.  So:
//   1. dilate the hole mask by a (2*(range+1)+1)^2 square and label its 8-connected components
//      (k_morph_bits + k_cc_label): hole pixels of different components are > 2*range+3 apart (Chebyshev),
//      while rings / neighbourhoods only reach across gaps of at most 2*range+1;
//   2. k_cluster_bbox / k_cluster_list: bounding box of the hole pixels of every component and the list of
//      components per frame; components whose window (bbox grown by range+1) exceeds the cluster kernel's
//      capacity are flagged `big`;
//   3. k_telea_clusters2 (k_inpaint_win.hip) marches every listed cluster on its own LDS window, one wave each,
//      and flags the ones whose queue overflowed;
//   4. k_split_bad builds the hole mask of the flagged clusters for the frame-window / whole-frame kernels.
#include "host_util.hpp"
#include "telea_common.hpp"

namespace vf {

// box planes (int32 [B,P], indexed by component root): xmin / ymin start at 0x7f7f7f7f, xmax / ymax at 0
__global__ void k_cluster_bbox(const uint8_t *__restrict__ bad, const int32_t *__restrict__ labels, int32_t *xmin, int32_t *ymin,
                               int32_t *xmax, int32_t *ymax, int h, int w)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    int P = h * w;
    const bool on = p < P && bad[b * (size_t)P + (p < P ? p : 0)] != 0;
    const int lab = on ? labels[b * (size_t)P + p] : -1;
    int y = p / w, x = p - y * w;
    // the hole pixels of a wave (64 consecutive pixels) mostly belong to one cluster: one set of atomics per cluster and wave instead of one
    // per pixel (the thousands of pixels of a big cluster all hit the same four words)
    unsigned long long active = __ballot(on);
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int r0 = __builtin_amdgcn_readlane(lab, leader);
        const unsigned long long same = __ballot(on && lab == r0);
        const bool mine = on && lab == r0;
        int x0 = mine ? x : 0x7fffffff, y0 = mine ? y : 0x7fffffff, x1 = mine ? x : -1, y1 = mine ? y : -1;
        for (int o = 32; o; o >>= 1) {
            x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
            x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
        }
        if ((int)(threadIdx.x & 63) == leader) {
            const size_t r = b * (size_t)P + r0;
            atomicMin(&xmin[r], x0); atomicMin(&ymin[r], y0); atomicMax(&xmax[r], x1); atomicMax(&ymax[r], y1);
        }
        active &= ~same;
    }
}

// list[b*P + k] = root of the k-th cluster of frame b that fits the cluster kernel; big[root] = 1 for the others
__global__ void k_cluster_list(const int32_t *__restrict__ labels, const int32_t *__restrict__ xmin, const int32_t *__restrict__ ymin,
                               const int32_t *__restrict__ xmax, const int32_t *__restrict__ ymax, int32_t *__restrict__ list,
                               int32_t *__restrict__ count, uint8_t *__restrict__ big, int range, int cells_cap, int h, int w)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    int P = h * w;
    if (p >= P) return;
    size_t i = b * (size_t)P + p;
    big[i] = 0;
    if (labels[i] != p || xmin[i] == 0x7f7f7f7f) return;
    if (telea_window_of_box(xmin[i], ymin[i], xmax[i], ymax[i], range).cells() > cells_cap) big[i] = 1;     // the unclipped window
    else { int k = atomicAdd(&count[b], 1); list[b * (size_t)P + k] = p; }
}

// after the LDS march: the roots still flagged `big` (window too large, or the queue of their window overflowed), compacted into `list`
__global__ void k_cluster_list_big(const int32_t *__restrict__ labels, const int32_t *__restrict__ xmin, const uint8_t *__restrict__ big,
                                   int32_t *__restrict__ list, int32_t *__restrict__ count, int h, int w)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    int P = h * w;
    if (p >= P) return;
    size_t i = b * (size_t)P + p;
    if (labels[i] != p || xmin[i] == 0x7f7f7f7f || !big[i]) return;
    int k = atomicAdd(&count[b], 1);
    list[b * (size_t)P + k] = p;
}

// bad_big = bad & big[root]
__global__ void k_split_bad(const uint8_t *__restrict__ bad, const int32_t *__restrict__ labels, const uint8_t *__restrict__ big,
                            uint8_t *__restrict__ bad_big, int P)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    if (p >= P) return;
    size_t i = b * (size_t)P + p;
    bad_big[i] = (uint8_t)(bad[i] && big[b * (size_t)P + labels[i]]);
}

struct ClusterScratch {
    uint8_t *dil;                       // [B, P] hole mask dilated by range + 1
    int32_t *labels;                    // [B, P]
    int32_t *xmin, *ymin, *xmax, *ymax; // [B, P] by root; xmin | ymin are one region, xmax | ymax another (one memset initialises each pair)
    int32_t *list;                      // [B, P]
    uint8_t *big, *bad_big;             // [B, P]
    int32_t *count;                     // [B]
};
static ClusterScratch inpaint_cl_scratch(ScratchLayout &L, int B, int h, int w)
{
    const size_t n = (size_t)B * h * w;
    ClusterScratch S;
    S.dil = L.take<uint8_t>(n, 256, "dil");
    S.labels = L.take<int32_t>(n, 256, "labels");
    S.xmin = L.take<int32_t>(2 * n, 256, "xmin_ymin");
    S.ymin = S.xmin ? S.xmin + n : nullptr;
    S.xmax = L.take<int32_t>(2 * n, 256, "xmax_ymax");
    S.ymax = S.xmax ? S.xmax + n : nullptr;
    S.list = L.take<int32_t>(n, 256, "list");
    S.big = L.take<uint8_t>(n, 256, "big");
    S.bad_big = L.take<uint8_t>(n, 256, "bad_big");
    S.count = L.take<int32_t>((size_t)B, 256, "count");
    return S;
}
size_t inpaint_cl_scratch_bytes(int B, int h, int w, ScratchRec *rec) { ScratchLayout L(nullptr, rec); inpaint_cl_scratch(L, B, h, w); return L.bytes(); }

bool inpaint_clusters_supported(int range) { return inpaint_big_supported(range); }     // the left-over clusters need k_inpaint_big.hip

// Marches every cluster that fits on its own window; *bad_big_out = hole mask of the clusters that were left over, *left = their roots
// (list / count per frame, in no particular order), labels and bounding boxes for launch_inpaint_big_clusters.
void launch_inpaint_clusters(float *img, const uint8_t *bad, int range, void *scratch, uint8_t **bad_big_out, ClusterPlanes *left, int B, int h, int w,
                             hipStream_t st)
{
    const int P = h * w;
    const size_t n = (size_t)B * P;
    ScratchLayout L(scratch);
    const ClusterScratch S = inpaint_cl_scratch(L, B, h, w);
    RowSpanSE se;
    const int R = range + 1;   // hole pixels interact only within Chebyshev distance 2*range+1; R = range would already separate them
    se.k = 2 * R + 1;
    for (int i = 0; i < se.k; i++) { se.lo[i] = (int8_t)(-R); se.hi[i] = (int8_t)R; }
    launch_morph(bad, S.dil, B, h, w, se, true, nullptr, nullptr, st);
    launch_cc_label(S.dil, S.labels, B, h, w, st);
    (void)hipMemsetAsync(S.xmin, 0x7f, n * 8, st);          // xmin, ymin
    (void)hipMemsetAsync(S.xmax, 0, n * 8, st);             // xmax, ymax
    (void)hipMemsetAsync(S.count, 0, (size_t)B * 4, st);
    dim3 g((P + 255) / 256, B);
    hipLaunchKernelGGL(k_cluster_bbox, g, dim3(256), 0, st, bad, S.labels, S.xmin, S.ymin, S.xmax, S.ymax, h, w);
    hipLaunchKernelGGL(k_cluster_list, g, dim3(256), 0, st, S.labels, S.xmin, S.ymin, S.xmax, S.ymax, S.list, S.count, S.big, range, inpaint_cluster_cells_cap(), h, w);
    launch_telea_clusters2(img, bad, S.labels, S.list, S.count, S.xmin, S.ymin, S.xmax, S.ymax, S.big, range, B, h, w, st);
    hipLaunchKernelGGL(k_split_bad, g, dim3(256), 0, st, bad, S.labels, S.big, S.bad_big, P);
    *bad_big_out = S.bad_big;
    if (left) {
        // the list of the clusters marched above is dead: it now takes the roots that are left
        (void)hipMemsetAsync(S.count, 0, (size_t)B * 4, st);
        hipLaunchKernelGGL(k_cluster_list_big, g, dim3(256), 0, st, S.labels, S.xmin, S.big, S.list, S.count, h, w);
        left->dil = S.dil; left->labels = S.labels; left->list = S.list; left->count = S.count; left->xmin = S.xmin; left->ymin = S.ymin; left->xmax = S.xmax; left->ymax = S.ymax;
    }
}

}  // namespace vf
