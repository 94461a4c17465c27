// Host-side plumbing shared by every translation unit that defines functions of the C ABI and by the launchers that cut a scratch buffer
// into planes: error reporting, the owning list of device allocations, the carver of the scratch layouts, and the OpenCV constant tables
// (Gaussian taps, structuring elements) that more than one modality builds.  Host only; nothing here launches a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vistaf_ftp.h"
#include "kernels.hpp"

struct vistaf_tempseg_handle;

namespace vf {

// records the calling thread's last-error text (vistaf_ftp_last_error) and returns `code`; defined in api.hip, used by every
// other translation unit of the ABI (stages.hip, api_hooks.hip, the read-outs)
int set_error(int code, const std::string &msg);

#define HIPCHK(x)                                                                                                     \
    do {                                                                                                              \
        const hipError_t e_ = (x);                                                                                    \
        if (e_ != hipSuccess) return vf::set_error(VISTAF_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));    \
    } while (0)
#define FCHK(x)                                                                                                                            \
    do {                                                                                                                                   \
        const hipfftResult r_ = (x);                                                                                                       \
        if (r_ != HIPFFT_SUCCESS) return vf::set_error(VISTAF_E_HIP, std::string(#x) + ": hipfft error " + std::to_string((int)r_));      \
    } while (0)

// a step of a create or a launcher that returns a VISTAF code: leave with it unless it is 0
#define TRY(x)                    \
    do {                          \
        const int rc_ = (x);      \
        if (rc_) return rc_;      \
    } while (0)

// What a vistaf_*_create holds its new handle in: Created<H> hd(new H(), vistaf_x_destroy).  Every early return (plain, TRY, HIPCHK, FCHK)
// then destroys the handle and what it owns so far; the last line of the create is `*out = hd.release()`.
template <class H>
using Created = std::unique_ptr<H, void (*)(H *)>;

// after a run of launches: 0, or VISTAF_E_HIP with "<what>: <the runtime's text>"
inline int launch_ok(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error(VISTAF_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The device buffers a handle owns; every buffer carries 256 bytes of padding behind its last element.
struct DeviceAllocs {
    std::vector<void *> ptrs;
    template <typename T>
    int alloc(T **p, size_t count)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T) + 256);
        if (e != hipSuccess) return set_error(VISTAF_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        ptrs.push_back(q);
        *p = (T *)q;
        return 0;
    }
    template <typename T>
    int upload(T **p, const T *host, size_t n)       // a new buffer of n elements holding a copy of host[0..n)
    {
        TRY(alloc(p, n));
        HIPCHK(hipMemcpy(*p, host, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    template <typename T>
    int upload(T **p, const std::vector<T> &host) { return upload(p, host.data(), host.size()); }
    void release(void *p)       // one buffer before the others; null and foreign pointers are ignored
    {
        const auto it = std::find(ptrs.begin(), ptrs.end(), p);
        if (p && it != ptrs.end()) { (void)hipFree(p); ptrs.erase(it); }
    }
    void free_all()
    {
        for (void *p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// Cuts one device buffer into aligned regions, in the order of the take() calls.  base == nullptr: counts only (pointers come back null), which
// is how every *_scratch_bytes() sizes the buffer its launcher carves: one function states a layout.  Offsets are rounded relative to base.
// base must be 256-byte aligned, as a hipMalloc pointer is: a launcher handed a pointer into the middle of a buffer aborts here (the assert is
// live in the shipped library) -- carve sub-buffers with take(), do not offset by hand.  rec: the regions, for the layout read-out of the tests.
struct ScratchRegion { const char *name; size_t offset, bytes, align; };
struct ScratchLayout {
    explicit ScratchLayout(void *base, ScratchRec *rec = nullptr) : base_((uint8_t *)base), rec_(rec) { assert(((uintptr_t)base & 255) == 0); }
    template <class T>
    T *take(size_t count, size_t align = 256, const char *name = nullptr)
    {
        off_ = (off_ + align - 1) & ~(align - 1);
        if (rec_) rec_->push_back({name, off_, count * sizeof(T), align});
        T *p = base_ ? (T *)(base_ + off_) : nullptr;
        off_ += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return off_; }      // end of the last region

private:
    uint8_t *base_;
    ScratchRec *rec_;
    size_t off_ = 0;
};

// the size query: the bytes layout(ScratchLayout &) takes, counted with a null base; rec: its regions
template <class Layout>
size_t scratch_bytes(Layout layout, ScratchRec *rec = nullptr)
{
    ScratchLayout L(nullptr, rec);
    layout(L);
    return L.bytes();
}

// The lazily built workspace of a handle: one buffer of `owner`, laid out by layout(ScratchLayout &), which returns the struct of its
// pointers.  Sizes it with a null layout, allocates, carves; *bufs and buf are set only when all of it succeeded.  A no-op once buf is set.
template <class Bufs, class Layout>
int ensure_carved(DeviceAllocs &owner, void *&buf, Bufs *bufs, Layout layout)
{
    if (buf) return 0;
    uint8_t *p = nullptr;
    TRY(owner.alloc(&p, scratch_bytes(layout)));
    ScratchLayout carve(p);
    *bufs = layout(carve);
    buf = p;
    return 0;
}

// ---- The host side of the read-outs with two plain functions and a workspace of the caller's (vistaf_X_workspace_bytes, vistaf_X_measure:
// outline, texture, match, centreline, lobes).  What their argument checks share; the checks of a read-out's own outputs, parameters and
// alignment sentences stay in its file.

// The sizes a read-out of the index plane takes (outline, centreline, lobes: coordinates are packed into 15 bits, edge slots into 31), and
// those of a read-out of the depth plane (texture, match; batch_text names the argument, batch or max_batch): the text of the refusal, or null
inline const char *plane_sizes_refusal(int h, int w, int batch, int max_contacts)
{
    if (h < 1 || h > 32767) return "h must be 1..32767";
    if (w < 1 || w > 32767) return "w must be 1..32767";
    if ((long long)h * w > 0x1fffffffll) return "h * w must be below 2^29";
    if (batch < 1 || batch > (1 << 24)) return "batch must be 1..2^24";
    if (max_contacts < 1 || max_contacts > VISTAF_MAX_CONTACTS) return "max_contacts must be 1..64";
    return nullptr;
}
inline const char *depth_sizes_refusal(int h, int w, int batch, const char *batch_text, int max_contacts)
{
    if (h < 1) return "h must be >= 1";
    if (w < 1) return "w must be >= 1";
    if ((long long)h * w > 0x7fffffffll) return "h * w must be below 2^31";
    if (batch < 1 || batch > (1 << 19)) return batch_text;
    if (max_contacts < 1 || max_contacts > VISTAF_MAX_CONTACTS) return "max_contacts must be 1..64";
    return nullptr;
}

// The answer of a vistaf_X_workspace_bytes: `refusal` is what the read-out's size checks said, need() the bytes, asked only for sizes they took
template <class Need>
int workspace_bytes_answer(size_t *bytes, const char *refusal, Need need)
{
    if (!bytes) return set_error(VISTAF_E_INVALID, "bytes is null");
    *bytes = 0;
    if (refusal) return set_error(VISTAF_E_INVALID, refusal);
    *bytes = need();
    return 0;
}

// the answer of a tier hook (test_hooks_centreline.h, test_hooks_lobes.h): 1 when in_lds(bw, bh) says a bw x bh box works in LDS, else 0
template <class Rule>
int tier_hook_answer(int bw, int bh, Rule in_lds)
{
    if (bw < 1 || bw > 32767) return set_error(VISTAF_E_INVALID, "bw must be 1..32767");
    if (bh < 1 || bh > 32767) return set_error(VISTAF_E_INVALID, "bh must be 1..32767");
    return in_lds(bw, bh) ? 1 : 0;
}

// the four inputs vistaf_ftp_contacts wrote: the text of the refusal, or null
inline const char *table_inputs_refusal(const void *d_contact_index, const void *d_contacts, const void *d_count, const void *d_mm_per_px)
{
    if (!d_contact_index) return "d_contact_index is null";
    if (!d_contacts) return "d_contacts is null";
    if (!d_count) return "d_count is null";
    if (!d_mm_per_px) return "d_mm_per_px is null";
    return nullptr;
}

// the caller's workspace against `need` bytes; sizer: the function that tells the caller how many
inline int workspace_ok(const void *d_workspace, size_t workspace_bytes, size_t need, const char *sizer)
{
    if (!d_workspace) return set_error(VISTAF_E_INVALID, "d_workspace is null");
    if ((uintptr_t)d_workspace & 255) return set_error(VISTAF_E_INVALID, "d_workspace must be 256-byte aligned");
    if (workspace_bytes < need) return set_error(VISTAF_E_INVALID, std::string("workspace_bytes is below what ") + sizer + " gives for these sizes");
    return 0;
}

// One frame of h x w pixels in an input format (VISTAF_FMT_*, include/vistaf_ftp.h): its bytes -- the frame stride of a batch -- and the
// pointer alignment the kernels of that format rely on, or the text of the refusal (then bytes and align are 0).  The one statement of the
// table in the header: api.hip refuses by it, launch_to_gray strides by it.
struct FrameLayout { size_t bytes; int align; const char *refusal; };
inline FrameLayout frame_layout(int format, int h, int w)
{
    if (h < 1 || w < 1) return {0, 0, "frame size below 1 x 1"};
    const size_t P = (size_t)h * (size_t)w;
    switch (format) {
    case VISTAF_FMT_GRAY_U8: return {P, 1, nullptr};
    case VISTAF_FMT_BGR_U8: return {3 * P, 1, nullptr};
    case VISTAF_FMT_GRAY_F16: return {2 * P, 2, nullptr};
    case VISTAF_FMT_BGR_F16: return {6 * P, 2, nullptr};
    case VISTAF_FMT_RGB_U8: return {3 * P, 1, nullptr};
    case VISTAF_FMT_BGRA_U8:
    case VISTAF_FMT_RGBA_U8: return {4 * P, 4, nullptr};
    case VISTAF_FMT_YUYV_U8:
    case VISTAF_FMT_UYVY_U8:
        if (w % 2) return {0, 0, format == VISTAF_FMT_YUYV_U8 ? "frame format YUYV needs an even width" : "frame format UYVY needs an even width"};
        return {2 * P, 4, nullptr};
    case VISTAF_FMT_NV12_U8:
        if (h % 2 || w % 2) return {0, 0, "frame format NV12 needs an even height and an even width"};
        return {P + P / 2, 1, nullptr};
    case VISTAF_FMT_BAYER_RGGB_U8:
    case VISTAF_FMT_BAYER_GRBG_U8:
    case VISTAF_FMT_BAYER_GBRG_U8:
    case VISTAF_FMT_BAYER_BGGR_U8:
        if (h < 2 || w < 2) return {0, 0, "frame format Bayer needs at least 2 x 2 pixels"};
        return {P, 1, nullptr};
    default: return {0, 0, "bad frame format: not one of VISTAF_FMT_* (0..13)"};
    }
}

inline int cv_round(double v) { return (int)std::nearbyint(v); }      // cvRound: half to even
inline int odd_up(int k) { return (k % 2) ? k : k + 1; }
inline dim3 grid1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// cv::GaussianBlur(src, (0, 0), sigma) on CV_32F: the ksize rule, and the float32 taps of cv::getGaussianKernel for that size.  Callers cap
// the size themselves (their kernels differ in the longest filter they take).
inline int gauss_ksize(double sigma) { return cv_round(sigma * 4 * 2 + 1) | 1; }
inline std::vector<float> gauss_taps(double sigma)
{
    const int n = gauss_ksize(sigma);
    std::vector<double> t(n);
    const double s2 = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; i++) { const double x = i - (n - 1) * 0.5; t[i] = std::exp(s2 * x * x); sum += t[i]; }
    std::vector<float> f(n);
    for (int i = 0; i < n; i++) f[i] = (float)(t[i] * (1.0 / sum));
    return f;
}

// cv::getStructuringElement(MORPH_ELLIPSE, (k, k)) as row spans, anchor at (k/2, k/2); k <= 33 (checked by the callers)
inline RowSpanSE ellipse_se(int k)
{
    RowSpanSE se;
    se.k = k;
    const int r = k / 2, c = k / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    for (int i = 0; i < 33; i++) { se.lo[i] = 1; se.hi[i] = -1; }
    for (int i = 0; i < k; i++) {
        const int dy = i - r;
        const int dx = cv_round(c * std::sqrt((r * r - dy * dy) * inv_r2));
        const int j1 = std::max(c - dx, 0), j2 = std::min(c + dx + 1, k);
        se.lo[i] = (int8_t)(j1 - c);
        se.hi[i] = (int8_t)(j2 - 1 - c);
    }
    return se;
}
// MORPH_RECT kx x ky: ky <= 33 rows of the same span
inline RowSpanSE rect_se(int kx, int ky)
{
    RowSpanSE se;
    se.k = ky;
    for (int i = 0; i < 33; i++) { se.lo[i] = (int8_t)(-(kx / 2)); se.hi[i] = (int8_t)(kx / 2); }
    return se;
}

// tempseg.hip, for the temperature session (tempsensor.hip): both workspaces of a segmentation session at once, and the two halves of
// the oriented blur (taps uploaded once, the blur itself asynchronous on taps already on the device)
int tempseg_prepare(vistaf_tempseg_handle *h);
int temp_blur_taps(double sigma_across, double sigma_along, float *d_kx, int &nx, float *d_ky, int &ny, hipStream_t st);
int temp_blur_apply(vistaf_tempseg_handle *h, const float *d_map, const uint8_t *d_roi, double angle_rad, const float *d_kx, int nx, const float *d_ky,
                    int ny, float *d_out, hipStream_t st);

}  // namespace vf
