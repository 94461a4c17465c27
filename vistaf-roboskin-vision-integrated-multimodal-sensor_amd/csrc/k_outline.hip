// Contact outline read-out (include_ext/vistaf_outline.h): boundary loops, holes, corner polyline, convex hull and caliper box of every contact,
// from the int8 index plane, table and counts vistaf_ftp_contacts wrote.  An extension, as the other per-contact read-outs: the reference has no
// counterpart.  The definition is in the header; tests/outline_helpers.py restates it with a walker that follows each loop edge by edge.
//
// Exact integer geometry; the hot part is ordering a loop, which is list ranking.  One workgroup per (frame, row) in all three launches:
//   k_outline_count  walks the row's box: its pixels, its boundary edges (a pixel owns the up to four edges it lies to the right of) and the
//                    leftmost / rightmost pixel of every box row (integer atomicMin / atomicMax, boundary pixels only).  The edge counts of the
//                    rows before k give row k its segment of the frame's edge slots: a frame has at most 4*h*w boundary edges over all rows.
//   k_outline_rank   walks the box again and gives every pixel the slot of its first edge (thread-major order: a workgroup scan of the threads'
//                    edge counts, which the first launch left, then a running count per thread) and every edge its start vertex; the
//                    successor -- a local function of the 2 x 2 block at the end vertex -- is found with one edge per thread, not one pixel,
//                    so that every lane works; then it ranks by pointer jumping: after round r an edge knows the smallest key among
//                    the 2^r edges from it on, how far ahead that edge is, and the edge 2^r ahead.  The key of a d = 0 edge is its pixel's
//                    row-major index, every other edge carries INT_MAX: every loop has d = 0 edges, the smallest names the loop, and on a
//                    positive loop it is the loop's first edge in (y, x, d) order.  ceil(log2(edges of the row)) rounds, the same for every
//                    thread of the workgroup.  Signed areas are integer atomic adds at the loop's first edge, one per wave and loop; counts,
//                    the principal loop, its length and corners are workgroup reductions.  The hull is two monotone chains over the row
//                    extremes (thread 0 on a stack in LDS, at most 2*(bh+1) points each way, fed in tiles of 1024 vertex rows); the calipers
//                    are O(m^2) over its m vertices, one edge per thread.
//   k_outline_poly   (only with polyline pointers) applies the capacity rule over the rows' CORNERS, scatters the principal loop's corners
//                    to their rank and compacts them with workgroup scans, in loop order.
// No memset, no float atomics, no host read-back: every double is computed once by one thread from exact integers, so two calls give the same
// bits and a frame's rows do not depend on the batch it is measured in.
#include <string>

#include "../../include_ext/vistaf_outline.h"
#include "contact_rows.hpp"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int OL_NT = 1024, OL_NW = OL_NT / 64;
constexpr int OL_NONE = 0x7fffffff;                       // key of an edge that is not a d = 0 edge; row extreme of a row without pixels
// The hull's stack.  What it holds is at every moment two strictly convex lattice chains, so its edges are distinct vectors, those of the first
// chain pointing down (or right), those of the second up (or left), with |dx| summing to at most 2w per chain and |dy| to at most h: a total
// L1 length below 2h + 4w + 8 <= 163850 for the sizes the read-out takes.  There are 4s vectors of L1 length s, so the 4900 shortest already
// measure 161700 together: fewer than 5000 points, whatever the mask.
constexpr int OL_HULL_CAP = 8192;
constexpr double OL_PI = 3.141592653589793, OL_HALF_PI = 1.5707963267948966;

// The workspace.  Per (frame, row): cnt (pixels, edges), tcnt (the edges every thread of the walk meets), meta (principal loop: key or -1, edges; the row's first edge slot, its edges), the row
// extremes.  Per frame: the slot of every pixel's first edge, and 4*h*w edge slots of next / vtx and two jump buffers of three int32 planes each (ahead, key, distance); the jump buffer a ranking does not end in serves as the area
// accumulators (its first plane) and as the corner scatter (its third), each row within its own edge slots.
struct OutlineBufs {
    int32_t *cnt, *tcnt, *meta, *rowlo, *rowhi, *off, *next;
    uint32_t *vtx;
    unsigned long long *jump[2];
};

OutlineBufs outline_scratch(ScratchLayout &L, int B, int h, int w, int K)
{
    const size_t rows = (size_t)B * K, P = (size_t)h * w;
    OutlineBufs bf;
    bf.cnt = L.take<int32_t>(rows * 2, 256, "row_counts");
    bf.tcnt = L.take<int32_t>(rows * OL_NT, 256, "thread_edge_counts");
    bf.meta = L.take<int32_t>(rows * 4, 256, "row_meta");
    bf.rowlo = L.take<int32_t>(rows * h, 256, "row_leftmost");
    bf.rowhi = L.take<int32_t>(rows * h, 256, "row_rightmost");
    bf.off = L.take<int32_t>((size_t)B * P, 256, "pixel_first_edge");
    bf.next = L.take<int32_t>((size_t)B * P * 4, 256, "edge_next");
    bf.vtx = L.take<uint32_t>((size_t)B * P * 4, 256, "edge_vertex");
    bf.jump[0] = L.take<unsigned long long>((size_t)B * P * 6, 256, "jump_0");
    bf.jump[1] = L.take<unsigned long long>((size_t)B * P * 6, 256, "jump_1");
    return bf;
}

// the three planes of a frame's jump buffer
struct OlJump {
    int32_t *ahead, *key, *dist;
    __device__ inline OlJump(unsigned long long *buf, size_t b, size_t P) : ahead((int32_t *)(buf + b * P * 6)), key(ahead + 4 * P), dist(ahead + 8 * P) {}
};

// header, step 2: the pixels right and left of edge (x, y, d), and the step of direction d
__device__ inline void ol_right(int x, int y, int d, int &px, int &py) { px = x - (d == 1 || d == 2); py = y - (d >= 2); }
__device__ inline void ol_left(int x, int y, int d, int &px, int &py) { px = x - (d >= 2); py = y - (d == 0 || d == 3); }
__device__ inline int ol_dx(int d) { return (d == 0) - (d == 2); }
__device__ inline int ol_dy(int d) { return (d == 1) - (d == 3); }
__device__ inline uint32_t ol_pack(int x, int y, int d) { return (uint32_t)x | ((uint32_t)y << 15) | ((uint32_t)d << 30); }
__device__ inline int ol_x(uint32_t v) { return (int)(v & 0x7fffu); }
__device__ inline int ol_y(uint32_t v) { return (int)((v >> 15) & 0x7fffu); }
__device__ inline int ol_d(uint32_t v) { return (int)(v >> 30); }
__device__ inline int ol_hx(uint32_t v) { return (int)(v & 0xffffu); }        // a hull point, x | y << 16
__device__ inline int ol_hy(uint32_t v) { return (int)(v >> 16); }

// The pixels of row k (header, step 1): index == k inside the clipped box; everything else is "not k"
struct OlRow {
    const int8_t *index;
    int w, k, x0, y0, x1, y1;
    __device__ inline OlRow(const int8_t *plane, int w_, int k_, const ContactBox &b) : index(plane), w(w_), k(k_), x0(b.x0), y0(b.y0), x1(b.x1), y1(b.y1)
    {
        if (!b.total()) { x0 = 0; x1 = -1; }
    }
    __device__ inline bool in(int x, int y) const { return x >= x0 && x <= x1 && y >= y0 && y <= y1 && index[(size_t)y * w + x] == k; }
    // the boundary edges pixel (x, y) of k owns, bit d: the pixel on the left of its d edge (above, right, below, left) is not k
    __device__ inline unsigned sides(int x, int y) const
    {
        return (in(x, y - 1) ? 0u : 1u) | (in(x + 1, y) ? 0u : 2u) | (in(x, y + 1) ? 0u : 4u) | (in(x - 1, y) ? 0u : 8u);
    }
};

__device__ inline long long ol_cross(int ox, int oy, int ax, int ay, int bx, int by)
{
    return (long long)(ax - ox) * (by - oy) - (long long)(ay - oy) * (bx - ox);
}

// atan2(p, q) folded into (-pi/2, pi/2]
__device__ inline double ol_dir(double p, double q)
{
    const double t = atan2(p, q);
    return t <= -OL_HALF_PI ? t + OL_PI : (t > OL_HALF_PI ? t - OL_PI : t);
}

__global__ __launch_bounds__(OL_NT) void k_outline_count(const int8_t *__restrict__ index, const double *__restrict__ contacts, const int32_t *__restrict__ count,
                                                         int h, int w, int K, int32_t *__restrict__ cnt, int32_t *__restrict__ tcnt, int32_t *__restrict__ rowlo, int32_t *__restrict__ rowhi)
{
    __shared__ unsigned long long red[16];
    const int b = blockIdx.x / K, k = blockIdx.x - b * K, tid = threadIdx.x;
    if (k >= clamp_count(count[b], K)) {
        if (tid < 2) cnt[(size_t)blockIdx.x * 2 + tid] = 0;
        return;
    }
    const ContactBox box(contacts + (size_t)blockIdx.x * VISTAF_NCONTACT, h, w);
    const OlRow row(index + (size_t)b * h * w, w, k, box);
    int32_t *lo = rowlo + (size_t)blockIdx.x * h, *hi = rowhi + (size_t)blockIdx.x * h;
    if (box.total())
        for (int y = box.y0 + tid; y <= box.y1; y += OL_NT) { lo[y] = OL_NONE; hi[y] = -1; }
    __syncthreads();
    unsigned long long npix = 0, nedge = 0;
    BoxWalk<OL_NT>(box, tid).each([&](int x, int y) {
        if (!row.in(x, y)) return;
        const unsigned s = row.sides(x, y);
        npix++;
        nedge += __popc(s);
        if (s & 8u) atomicMin(&lo[y], x);
        if (s & 2u) atomicMax(&hi[y], x);
    });
    tcnt[(size_t)blockIdx.x * OL_NT + tid] = (int32_t)nedge;
    npix = block_sum(npix, red);
    nedge = block_sum(nedge, red);
    if (tid == 0) {
        cnt[(size_t)blockIdx.x * 2] = (int32_t)npix;
        cnt[(size_t)blockIdx.x * 2 + 1] = (int32_t)nedge;
    }
}

__global__ __launch_bounds__(OL_NT) void k_outline_rank(const int8_t *__restrict__ index, const double *__restrict__ contacts, const int32_t *__restrict__ count,
                                                        const double *__restrict__ mm_per_px, int h, int w, int K, OutlineBufs bf, double *__restrict__ outlines)
{
    __shared__ unsigned long long red[16];
    __shared__ int wtot[OL_NW];
    __shared__ int hull_m;
    __shared__ int tile[2 * OL_NT];
    __shared__ uint32_t H[OL_HULL_CAP];                      // hull points, x | y << 16
    const int b = blockIdx.x / K, k = blockIdx.x - b * K, tid = threadIdx.x, lane = tid & 63;
    double *out = outlines + (size_t)blockIdx.x * VISTAF_NOUTLINE;
    if (nan_row(k >= clamp_count(count[b], K), out, VISTAF_NOUTLINE)) return;
    const size_t P = (size_t)h * w;
    int seg = 0;                                             // the row's first edge slot: the edges of the rows before it
    for (int j = 0; j < k; j++) seg += bf.cnt[((size_t)b * K + j) * 2 + 1];
    const int npix = bf.cnt[(size_t)blockIdx.x * 2], E = bf.cnt[(size_t)blockIdx.x * 2 + 1];
    int32_t *meta = bf.meta + (size_t)blockIdx.x * 4;
    if (npix == 0) {
        if (tid < VISTAF_NOUTLINE) out[tid] = tid <= VISTAF_OUTLINE_EDGES_ALL || (tid >= VISTAF_OUTLINE_CORNERS && tid <= VISTAF_OUTLINE_HULL_VERTICES) ? 0.0 : nan64();
        if (tid == 0) { meta[0] = -1; meta[1] = 0; meta[2] = seg; meta[3] = 0; }
        return;
    }
    const ContactBox box(contacts + (size_t)blockIdx.x * VISTAF_NCONTACT, h, w);
    const OlRow row(index + b * P, w, k, box);
    const BoxWalk<OL_NT> walk(box, tid);
    int32_t *off = bf.off + b * P, *next = bf.next + b * P * 4;
    uint32_t *vtx = bf.vtx + b * P * 4;

    // ---- the slot of every pixel's first edge, thread-major (the threads' edge counts are k_outline_count's: the same walk), and every edge's
    // start vertex, direction and key
    int total;
    int at = seg + block_excl_scan<OL_NW>(bf.tcnt[(size_t)blockIdx.x * OL_NT + tid], wtot, total);
    int rounds = 0;
    while ((1 << rounds) < E) rounds++;
    const OlJump j0(bf.jump[0], b, P);
    walk.each([&](int px, int py) {
        if (!row.in(px, py)) return;
        const unsigned s = row.sides(px, py);
        const int p = py * w + px;
        off[p] = at;
        for (int d = 0; d < 4; d++) {
            if (!((s >> d) & 1u)) continue;
            vtx[at] = ol_pack(px + (d == 1 || d == 2), py + (d >= 2), d);
            j0.key[at] = d == 0 ? p : OL_NONE;
            j0.dist[at] = 0;
            at++;
        }
    });
    __syncthreads();

    // ---- every edge's successor (header, step 3), one edge per thread
    for (int e = seg + tid; e < seg + E; e += OL_NT) {
        const uint32_t q = vtx[e];
        const int d = ol_d(q), qx = ol_x(q) + ol_dx(d), qy = ol_y(q) + ol_dy(d);
        int ax, ay, nd;
        ol_left(qx, qy, d, ax, ay);
        if (row.in(ax, ay)) nd = (d + 3) & 3;
        else {
            ol_right(qx, qy, d, ax, ay);
            nd = row.in(ax, ay) ? d : (d + 1) & 3;
        }
        ol_right(qx, qy, nd, ax, ay);                          // the pixel that owns the successor
        const int en = off[(size_t)ay * w + ax] + __popc(row.sides(ax, ay) & ((1u << nd) - 1u));
        next[e] = en;
        j0.ahead[e] = en;
    }
    __syncthreads();

    // ---- pointer jumping: the smallest key of the 2^r edges from e on, the distance to its edge, the edge 2^r ahead
    for (int r = 0; r < rounds; r++) {
        const OlJump src(bf.jump[r & 1], b, P), dst(bf.jump[(r + 1) & 1], b, P);
        for (int e = seg + tid; e < seg + E; e += OL_NT) {
            const int a = src.ahead[e];
            int key = src.key[e], dist = src.dist[e];
            const int key2 = src.key[a], dist2 = src.dist[a];
            if (key2 < key) { key = key2; dist = dist2 + (1 << r); }
            dst.ahead[e] = src.ahead[a];
            dst.key[e] = key;
            dst.dist[e] = dist;
        }
        __syncthreads();
    }
    const OlJump fin(bf.jump[rounds & 1], b, P), spare(bf.jump[(rounds + 1) & 1], b, P);
    int32_t *acc = spare.ahead;                                // |A2| <= 2*h*w <= 2^30: an int32, at the slot of the loop's first edge

    // ---- twice-areas (int32: |A2| <= 2*h*w <= 2^30): the first edge of a loop (distance 0) clears its accumulator, every edge adds x*y' - x'*y there, one add per wave and loop
    for (int e = seg + tid; e < seg + E; e += OL_NT)
        if (fin.dist[e] == 0) acc[e] = 0;
    __syncthreads();
    for (int base = seg; base < seg + E; base += OL_NT) {
        const int e = base + tid;
        bool pending = e < seg + E;
        int first = 0;
        int v = 0;
        if (pending) {
            const uint32_t q = vtx[e];
            const int d = ol_d(q);
            first = off[fin.key[e]];
            v = d == 0 ? -ol_y(q) : (d == 1 ? ol_x(q) : (d == 2 ? ol_y(q) : -ol_x(q)));
        }
        for (unsigned long long todo = __ballot(pending); todo; todo = __ballot(pending)) {
            const int leader = __ffsll((long long)todo) - 1;
            const int f = __builtin_amdgcn_readlane(first, leader);
            const bool same = pending && first == f;
            const int sum = wave_sum(same ? v : 0);
            if (lane == leader) atomicAdd(&acc[f], sum);
            pending = pending && !same;
        }
    }
    __syncthreads();

    // ---- loops: pieces, holes, the principal loop (largest A2, then the smallest key), its edges and corners
    unsigned long long pieces = 0, holes = 0, best = 0;
    for (int e = seg + tid; e < seg + E; e += OL_NT)
        if (fin.dist[e] == 0) {
            const long long a2 = (long long)ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&acc[e]);      // written by atomics: read where they landed
            if (a2 > 0) {
                pieces++;
                const unsigned long long cand = ((unsigned long long)(a2 / 2) << 32) | (0xffffffffu - (uint32_t)fin.key[e]);
                best = cand > best ? cand : best;
            } else holes++;
        }
    pieces = block_sum(pieces, red);
    holes = block_sum(holes, red);
    best = block_max_u64(best, red);
    const int pkey = (int)(0xffffffffu - (uint32_t)best);
    unsigned long long far = 0, ncorner = 0;
    for (int e = seg + tid; e < seg + E; e += OL_NT)
        if (fin.key[e] == pkey) {
            const unsigned long long dist = (unsigned long long)fin.dist[e];
            far = dist > far ? dist : far;
            ncorner += ol_d(vtx[next[e]]) != ol_d(vtx[e]) ? 1u : 0u;
        }
    far = block_max_u64(far, red);
    ncorner = block_sum(ncorner, red);

    // ---- hull: the candidate points of every vertex row, tile by tile through LDS; thread 0 runs the two monotone chains on a stack in LDS
    const int nrows = box.bh + 1, ntiles = (nrows + OL_NT - 1) / OL_NT;
    const int32_t *lo = bf.rowlo + (size_t)blockIdx.x * h, *hi = bf.rowhi + (size_t)blockIdx.x * h;
    auto load_tile = [&](int t) {                              // vertex row i of the box: the extremes of the pixel rows above and below it
        const int i = t * OL_NT + tid, y = box.y0 + i;
        int l = OL_NONE, r = -1;
        if (i < nrows) {
            if (i > 0 && hi[y - 1] >= 0) { l = lo[y - 1]; r = hi[y - 1]; }
            if (i < box.bh && hi[y] >= 0) { l = lo[y] < l ? lo[y] : l; r = hi[y] > r ? hi[y] : r; }
        }
        __syncthreads();
        tile[2 * tid] = l;
        tile[2 * tid + 1] = r + 1;
        __syncthreads();
    };
    int n = 0, ax = 0, ay = 0, bx = 0, by = 0, last = 0;       // thread 0's: the stack's size, its two top points, the last row with points
    auto add = [&](int x, int y, int floor) {
        while (n >= floor && ol_cross(ax, ay, bx, by, x, y) <= 0) {
            n--;
            bx = ax; by = ay;
            if (n >= 2) { const uint32_t v = H[n - 2]; ax = (int)(v & 0xffffu); ay = (int)(v >> 16); }
        }
        H[n < OL_HULL_CAP ? n : OL_HULL_CAP - 1] = (uint32_t)x | ((uint32_t)y << 16);
        n++;
        ax = bx; ay = by; bx = x; by = y;
    };
    for (int t = 0; t < ntiles; t++) {
        load_tile(t);
        if (tid == 0)
            for (int j = 0, i = t * OL_NT; j < OL_NT && i < nrows; j++, i++) {
                if (tile[2 * j] == OL_NONE) continue;
                add(tile[2 * j], box.y0 + i, 2);
                add(tile[2 * j + 1], box.y0 + i, 2);
                last = i;
            }
    }
    const int floor = n + 1;
    for (int t = ntiles - 1; t >= 0; t--) {
        load_tile(t);
        if (tid == 0) {
            int j = nrows - t * OL_NT < OL_NT ? nrows - t * OL_NT - 1 : OL_NT - 1;
            for (int i = t * OL_NT + j; j >= 0; j--, i--) {
                if (tile[2 * j] == OL_NONE) continue;
                if (i != last) add(tile[2 * j + 1], box.y0 + i, floor);
                add(tile[2 * j], box.y0 + i, floor);
            }
            if (t == 0) hull_m = n - 1;                        // the last point is the first again
        }
    }
    __syncthreads();
    const int m = hull_m;
    unsigned long long ha2 = 0, area_bits = ~0ull, across_bits = ~0ull, d2max = 0;
    for (int i = tid; i < m; i += OL_NT) {
        const int xi = ol_hx(H[i]), yi = ol_hy(H[i]), in = i + 1 < m ? i + 1 : 0;
        const long long ex = ol_hx(H[in]) - xi, ey = ol_hy(H[in]) - yi, L2 = ex * ex + ey * ey;
        ha2 += (unsigned long long)((long long)xi * ol_hy(H[in]) - (long long)ol_hx(H[in]) * yi);
        long long amin = 0, amax = 0, cmax = 0;
        for (int j = 0; j < m; j++) {
            const long long dx = ol_hx(H[j]) - xi, dy = ol_hy(H[j]) - yi, a = dx * ex + dy * ey, c = ex * dy - ey * dx, d2 = dx * dx + dy * dy;
            amin = a < amin ? a : amin;
            amax = a > amax ? a : amax;
            cmax = c > cmax ? c : cmax;
            if (j > i && (unsigned long long)d2 > d2max) d2max = (unsigned long long)d2;
        }
        const double area = (double)(amax - amin) * (double)cmax / (double)L2, across = (double)cmax / sqrt((double)L2);
        const unsigned long long ab = (unsigned long long)__double_as_longlong(area), cb = (unsigned long long)__double_as_longlong(across);
        area_bits = ab < area_bits ? ab : area_bits;          // positive doubles order as their bits
        across_bits = cb < across_bits ? cb : across_bits;
    }
    ha2 = block_sum(ha2, red);
    area_bits = block_min_u64(area_bits, red);
    across_bits = block_min_u64(across_bits, red);
    d2max = block_max_u64(d2max, red);
    // the first edge of that area, the first pair of that distance
    unsigned long long box_i = ~0ull, pair = ~0ull;
    for (int i = tid; i < m; i += OL_NT) {
        const int xi = ol_hx(H[i]), yi = ol_hy(H[i]), in = i + 1 < m ? i + 1 : 0;
        const long long ex = ol_hx(H[in]) - xi, ey = ol_hy(H[in]) - yi, L2 = ex * ex + ey * ey;
        long long amin = 0, amax = 0, cmax = 0;
        for (int j = 0; j < m; j++) {
            const long long dx = ol_hx(H[j]) - xi, dy = ol_hy(H[j]) - yi, a = dx * ex + dy * ey, c = ex * dy - ey * dx;
            amin = a < amin ? a : amin;
            amax = a > amax ? a : amax;
            cmax = c > cmax ? c : cmax;
            if (j > i && pair == ~0ull && (unsigned long long)(dx * dx + dy * dy) == d2max) pair = ((unsigned long long)i << 32) | (unsigned)j;
        }
        const double area = (double)(amax - amin) * (double)cmax / (double)L2;
        if (box_i == ~0ull && (unsigned long long)__double_as_longlong(area) == area_bits) box_i = (unsigned long long)i;
    }
    box_i = block_min_u64(box_i, red);
    pair = block_min_u64(pair, red);

    if (tid == 0) {
        const double s = mm_per_px[b];
        const long long a2 = (long long)ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&acc[off[pkey]]);
        const int edges = (int)far + 1;
        for (int j = 0; j < VISTAF_NOUTLINE; j++) out[j] = nan64();
        out[VISTAF_OUTLINE_PIXELS] = (double)npix;
        out[VISTAF_OUTLINE_PIECES] = (double)pieces;
        out[VISTAF_OUTLINE_HOLES] = (double)holes;
        out[VISTAF_OUTLINE_EDGES] = (double)edges;
        out[VISTAF_OUTLINE_EDGES_ALL] = (double)E;
        out[VISTAF_OUTLINE_PERIMETER_MM] = (double)edges * s;
        out[VISTAF_OUTLINE_ENCLOSED_PIXELS] = (double)(a2 / 2);
        out[VISTAF_OUTLINE_CORNERS] = (double)ncorner;
        out[VISTAF_OUTLINE_CORNERS_WRITTEN] = 0.0;
        out[VISTAF_OUTLINE_HULL_VERTICES] = (double)m;
        const double half = (double)(long long)ha2 / 2.0;
        out[VISTAF_OUTLINE_HULL_AREA_MM2] = half * s * s;
        out[VISTAF_OUTLINE_SOLIDITY] = (double)npix / half;
        const int fi = (int)(pair >> 32), fj = (int)(uint32_t)pair;
        out[VISTAF_OUTLINE_MAX_FERET_MM] = sqrt((double)d2max) * s;
        out[VISTAF_OUTLINE_MAX_FERET_ANGLE_RAD] = ol_dir((double)(ol_hy(H[fj]) - ol_hy(H[fi])), (double)(ol_hx(H[fj]) - ol_hx(H[fi])));
        out[VISTAF_OUTLINE_MIN_FERET_MM] = __longlong_as_double((long long)across_bits) * s;
        const int i = (int)box_i, in = i + 1 < m ? i + 1 : 0, xi = ol_hx(H[i]), yi = ol_hy(H[i]);
        const long long ex = ol_hx(H[in]) - xi, ey = ol_hy(H[in]) - yi, L2 = ex * ex + ey * ey;
        long long amin = 0, amax = 0, cmax = 0;
        for (int j = 0; j < m; j++) {
            const long long dx = ol_hx(H[j]) - xi, dy = ol_hy(H[j]) - yi, a = dx * ex + dy * ey, c = ex * dy - ey * dx;
            amin = a < amin ? a : amin;
            amax = a > amax ? a : amax;
            cmax = c > cmax ? c : cmax;
        }
        const double root = sqrt((double)L2), along = (double)(amax - amin) / root, across = (double)cmax / root;
        out[VISTAF_OUTLINE_BOX_CX] = (double)xi + (double)(ex * (amin + amax) - ey * cmax) / (double)(2 * L2);
        out[VISTAF_OUTLINE_BOX_CY] = (double)yi + (double)(ey * (amin + amax) + ex * cmax) / (double)(2 * L2);
        out[VISTAF_OUTLINE_BOX_LENGTH_MM] = (along >= across ? along : across) * s;
        out[VISTAF_OUTLINE_BOX_WIDTH_MM] = (along >= across ? across : along) * s;
        out[VISTAF_OUTLINE_BOX_ANGLE_RAD] = along >= across ? ol_dir((double)ey, (double)ex) : ol_dir((double)ex, (double)-ey);
        meta[0] = pkey; meta[1] = edges; meta[2] = seg; meta[3] = E;
    }
}

__global__ __launch_bounds__(OL_NT) void k_outline_poly(const int32_t *__restrict__ count, int h, int w, int K, int max_vertices, OutlineBufs bf,
                                                        double *__restrict__ outlines, int32_t *__restrict__ vertices, int32_t *__restrict__ offsets)
{
    __shared__ int wtot[OL_NW];
    const int b = blockIdx.x / K, k = blockIdx.x - b * K, tid = threadIdx.x;
    const int kk = clamp_count(count[b], K);
    const RowCapacity cap = row_capacity(outlines, VISTAF_NOUTLINE, VISTAF_OUTLINE_CORNERS, b, K, k, kk, max_vertices);
    const int before = cap.before, written = cap.written;
    if (tid == 0) {
        if (k == 0) offsets[(size_t)b * (K + 1)] = 0;
        offsets[(size_t)b * (K + 1) + k + 1] = before + written;
        if (k < kk) outlines[(size_t)blockIdx.x * VISTAF_NOUTLINE + VISTAF_OUTLINE_CORNERS_WRITTEN] = (double)written;
    }
    if (!written) return;
    const size_t P = (size_t)h * w;
    const int32_t *meta = bf.meta + (size_t)blockIdx.x * 4;
    const int pkey = meta[0], L = meta[1], seg = meta[2], E = meta[3];
    int rounds = 0;
    while ((1 << rounds) < E) rounds++;
    const OlJump fin(bf.jump[rounds & 1], b, P), spare(bf.jump[(rounds + 1) & 1], b, P);
    const int32_t *next = bf.next + b * P * 4;
    const uint32_t *vtx = bf.vtx + b * P * 4;
    uint32_t *slot = (uint32_t *)spare.dist + seg;             // L <= E slots: the vertex at rank q of the loop if it is a corner
    // the end vertex of an edge of rank r is the start of the edge of rank r + 1, a corner when the direction changes there
    for (int e = seg + tid; e < seg + E; e += OL_NT)
        if (fin.key[e] == pkey) {
            const int dist = fin.dist[e], rank = dist ? L - dist : 0, q = rank + 1 < L ? rank + 1 : 0;
            const uint32_t v = vtx[e], vn = vtx[next[e]];
            slot[q] = ol_d(vn) != ol_d(v) ? (vn & 0x3fffffffu) : 0xffffffffu;
        }
    __syncthreads();
    int32_t *dst = vertices + ((size_t)b * max_vertices + before) * 2;
    int done = 0;
    for (int base = 0; base < L; base += OL_NT) {
        const int q = base + tid;
        const uint32_t v = q < L ? slot[q] : 0xffffffffu;
        int total;
        const int at = done + block_excl_scan<OL_NW>(v != 0xffffffffu ? 1 : 0, wtot, total);
        if (v != 0xffffffffu) {
            dst[2 * at] = ol_x(v);
            dst[2 * at + 1] = ol_y(v);
        }
        done += total;
    }
}

}  // namespace

namespace vf {

size_t outline_scratch_bytes(int B, int h, int w, int K, ScratchRec *rec)
{
    return scratch_bytes([&](ScratchLayout &L) { return outline_scratch(L, B, h, w, K); }, rec);
}

}  // namespace vf

extern "C" {

int vistaf_outline_workspace_bytes(int h, int w, int batch, int max_contacts, size_t *bytes)
{
    return workspace_bytes_answer(bytes, plane_sizes_refusal(h, w, batch, max_contacts), [&] { return outline_scratch_bytes(batch, h, w, max_contacts, nullptr); });
}

int vistaf_outline_measure(const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count, const double *d_mm_per_px, int batch,
                           int h, int w, int max_contacts, int max_vertices, double *d_outlines, int32_t *d_vertices, int32_t *d_offsets,
                           void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (const char *why = table_inputs_refusal(d_contact_index, d_contacts, d_count, d_mm_per_px)) return set_error(VISTAF_E_INVALID, why);
    if (!d_outlines) return set_error(VISTAF_E_INVALID, "d_outlines is null");
    if (const char *why = plane_sizes_refusal(h, w, batch, max_contacts)) return set_error(VISTAF_E_INVALID, why);
    if (max_vertices < 0) return set_error(VISTAF_E_INVALID, "max_vertices must be >= 0");
    if (!d_vertices && d_offsets) return set_error(VISTAF_E_INVALID, "d_vertices is null although d_offsets is given");
    if (((uintptr_t)d_contacts | (uintptr_t)d_mm_per_px | (uintptr_t)d_outlines) & 7) return set_error(VISTAF_E_INVALID, "d_contacts, d_mm_per_px and d_outlines must be 8-byte aligned");
    if (((uintptr_t)d_count | (uintptr_t)d_vertices | (uintptr_t)d_offsets) & 3) return set_error(VISTAF_E_INVALID, "d_count, d_vertices and d_offsets must be 4-byte aligned");
    TRY(workspace_ok(d_workspace, workspace_bytes, outline_scratch_bytes(batch, h, w, max_contacts, nullptr), "vistaf_outline_workspace_bytes"));
    ScratchLayout L(d_workspace);
    const OutlineBufs bf = outline_scratch(L, batch, h, w, max_contacts);
    const dim3 grid((unsigned)(batch * max_contacts)), block(OL_NT);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_outline_count, grid, block, 0, st, d_contact_index, d_contacts, d_count, h, w, max_contacts, bf.cnt, bf.tcnt, bf.rowlo, bf.rowhi);
    hipLaunchKernelGGL(k_outline_rank, grid, block, 0, st, d_contact_index, d_contacts, d_count, d_mm_per_px, h, w, max_contacts, bf, d_outlines);
    if (d_vertices && d_offsets)
        hipLaunchKernelGGL(k_outline_poly, grid, block, 0, st, d_count, h, w, max_contacts, max_vertices, bf, d_outlines, d_vertices, d_offsets);
    return launch_ok("k_outline");
}

}  // extern "C"
