// Stand-alone host check of how a handle of the C ABI is owned (csrc/host_util.hpp): the create guard, DeviceAllocs and ensure_carved on their
// failure paths, for a run under the host sanitizers.  It runs where there is no device, so the first hipMalloc fails: that is the failure
// path every vistaf_*_create takes when an allocation fails half way.  Nothing here launches a kernel.  Build and run (no GPU needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o handle_host_check tests/diag/handle_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./handle_host_check
#include <cstdio>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/host_util.hpp"

static std::string g_last;
namespace vf {
int set_error(int code, const std::string &msg) { g_last = msg; return code; }
}  // namespace vf
using namespace vf;

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

// a handle as the library's are: plain fields, the device memory in a DeviceAllocs, a destroy that frees both
struct toy_handle {
    int n = 0;
    float *plane = nullptr;
    void *buf = nullptr;
    struct Bufs { float *a; double *b; } bf = {};
    DeviceAllocs mem;
};
static int g_destroyed = 0;
static void toy_destroy(toy_handle *t)
{
    if (!t) return;
    g_destroyed++;
    t->mem.free_all();
    delete t;
}
static toy_handle::Bufs toy_scratch(ScratchLayout &L, int n)
{
    toy_handle::Bufs bf;
    bf.a = L.take<float>((size_t)n, 256, "a");
    bf.b = L.take<double>((size_t)n, 256, "b");
    return bf;
}

// shaped like every vistaf_*_create: checks, new into the guard, steps that may fail, release
static int toy_create(int n, bool allocate, toy_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument");
    if (n < 1) return set_error(VISTAF_E_INVALID, "n must be >= 1");
    Created<toy_handle> t(new toy_handle(), toy_destroy);
    t->n = n;
    if (n > 1000) return set_error(VISTAF_E_INVALID, "n must be <= 1000");      // a plain return after new
    if (allocate) TRY(t->mem.alloc(&t->plane, (size_t)n));
    *out = t.release();
    return 0;
}

int main()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        std::printf("handle host check skipped: it checks the path of a failing hipMalloc and this machine has a device\n");
        return 0;
    }
    toy_handle *t = nullptr;
    // refused before new: nothing to destroy
    EXPECT(toy_create(0, true, &t) == VISTAF_E_INVALID && t == nullptr && g_destroyed == 0);
    // a plain return and a failing allocation between new and release: destroyed exactly once, *out untouched
    EXPECT(toy_create(1001, true, &t) == VISTAF_E_INVALID && t == nullptr && g_destroyed == 1);
    EXPECT(toy_create(8, true, &t) == VISTAF_E_HIP && t == nullptr && g_destroyed == 2);
    EXPECT(g_last.rfind("hipMalloc: ", 0) == 0);
    // released: the guard does not destroy, the caller's destroy does
    EXPECT(toy_create(8, false, &t) == 0 && t != nullptr && g_destroyed == 2 && t->n == 8 && t->mem.ptrs.empty());
    // upload on the failing path: no pointer handed out, nothing recorded
    const std::vector<float> taps = {0.25f, 0.5f, 0.25f};
    float *d_taps = nullptr;
    EXPECT(t->mem.upload(&d_taps, taps) == VISTAF_E_HIP && d_taps == nullptr && t->mem.ptrs.empty());
    // ensure_carved with a failing allocation: buf stays null, the struct untouched, and the layout was only asked for its size
    int sized = 0, carved = 0;
    auto layout = [&](ScratchLayout &L) {
        const toy_handle::Bufs bf = toy_scratch(L, t->n);
        (bf.a == nullptr ? sized : carved)++;
        return bf;
    };
    EXPECT(ensure_carved(t->mem, t->buf, &t->bf, layout) == VISTAF_E_HIP);
    EXPECT(t->buf == nullptr && t->bf.a == nullptr && t->bf.b == nullptr && t->mem.ptrs.empty() && sized == 1 && carved == 0);
    // once a buffer is there it is a no-op: the layout is not asked again
    alignas(256) static unsigned char room[1024];
    t->buf = room;
    EXPECT(ensure_carved(t->mem, t->buf, &t->bf, layout) == 0 && t->buf == room && sized == 1 && carved == 0);
    t->buf = nullptr;
    // what it would carve: sized with a null base, carved from a buffer of exactly that size
    ScratchLayout size(nullptr);
    toy_scratch(size, t->n);
    EXPECT(size.bytes() == 256 + 8 * sizeof(double) && size.bytes() <= sizeof(room));
    ScratchLayout carve(room);
    const toy_handle::Bufs bf = toy_scratch(carve, t->n);
    EXPECT((unsigned char *)bf.a == room && (unsigned char *)bf.b == room + 256 && carve.bytes() == size.bytes());
    toy_destroy(t);
    EXPECT(g_destroyed == 3);
    toy_destroy(nullptr);
    EXPECT(g_destroyed == 3);
    std::printf("handle host check ok\n");
    return 0;
}
