// Per-thread error record and library info for libpcc_structural.so.
#include "pcc_common.hpp"

#include <atomic>
#include <cstdarg>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace {
thread_local int t_status = 0;
thread_local char t_msg[320] = "";
}  // namespace

#include "pcc_test_hooks.h"
namespace {
int g_tuning[PCC_TUNE_KEYS] = {};
static_assert(PCC_TUNE_OCCUPANCY_PATH < PCC_TUNE_KEYS, "a tuning key outside the table");
}

namespace pcc {
// compute units of the CURRENT device (cached per device: a process may drive several)
int device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
            (void)hipGetLastError();
            v = 0;
        }
        cache[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}
int device_cus_or(int fallback) {
    const int cus = device_cus();
    return cus > 0 ? cus : fallback;
}

int tuning(int key) { return key >= 0 && key < PCC_TUNE_KEYS ? __atomic_load_n(&g_tuning[key], __ATOMIC_RELAXED) : 0; }
void set_error(int status, const char *what) {
    t_status = status;
    std::strncpy(t_msg, what ? what : "", sizeof t_msg - 1);
    t_msg[sizeof t_msg - 1] = '\0';
}
void clear_error() {
    t_status = 0;
    t_msg[0] = '\0';
}
int invalidf(const char *fmt, ...) {
    char buf[256];
    va_list args;
    va_start(args, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, args);
    va_end(args);
    return invalid(buf);
}
int check_list_sizes(const char *name, int b, int c, int n, int m, int k) {
    if (b < 0 || c < 1 || n < 1 || m < 0 || k < 1) return invalidf("%s: bad size", name);
    if (b > 65535) return invalidf("%s: batch too large", name);
    if ((long long)m * k > 0x7fffffffLL) return invalidf("%s: list too long (m * k >= 2^31)", name);
    return PCC_OK;
}
int check_out_slice(const char *name, int c, int out_c, int out_c0) {
    if (out_c0 < 0 || (long long)out_c0 + c > out_c)
        return invalidf("%s: channels out_c0 .. out_c0 + c - 1 are not inside out_c", name);
    return PCC_OK;
}
int zero_async(void *p, size_t bytes, hipStream_t st, const char *what) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    if (e == hipSuccess) return PCC_OK;
    (void)hipGetLastError();
    set_error((int)e, what);
    return (int)e;
}

namespace {
struct ProfRec {
    const char *name;
    hipEvent_t a, b;
};
int g_prof_mode = 0;  // 0 off, 1 every kernel launch, 2 only the coarse scopes (launch sequences)
std::mutex g_prof_mu;
std::vector<ProfRec> g_prof;
void prof_clear() {
    for (auto &r : g_prof) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_prof.clear();
}
}  // namespace

namespace {
std::mutex g_pool_mu;
hipMemPool_t g_pools[64] = {};
bool g_pool_failed[64] = {};
hipMemPool_t device_pool() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!g_pools[dev] && !g_pool_failed[dev]) {
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t pool = nullptr;
        if (hipMemPoolCreate(&pool, &props) == hipSuccess) {
            uint64_t keep = kPoolKeepBytes;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
            g_pools[dev] = pool;
        } else {
            (void)hipGetLastError();
            g_pool_failed[dev] = true;  // fall back to the default pool, untouched
        }
    }
    return g_pools[dev];
}
}  // namespace

hipError_t ws_malloc(void **p, size_t bytes, hipStream_t st) {
    hipMemPool_t pool = device_pool();
    hipError_t e = pool ? hipMallocFromPoolAsync(p, bytes, pool, st) : hipMallocAsync(p, bytes, st);
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        return e;
    }
    // PCC_WS_POISON=1 (test runs): every workspace starts as 0xFF bytes -- NaN as a float, -1 as an index -- so a kernel
    // that reads scratch nobody wrote shows up as a NaN / a fault instead of passing on whatever the pool held before
    static const bool poison = [] {
        const char *v = std::getenv("PCC_WS_POISON");
        return v && v[0] == '1';
    }();
    if (poison) (void)hipMemsetAsync(*p, 0xFF, bytes, st);
    return e;
}
hipError_t ws_free(void *p, hipStream_t st) { return p ? hipFreeAsync(p, st) : hipSuccess; }

bool profiling() { return g_prof_mode != 0; }
ProfScope::ProfScope(const char *kernel, hipStream_t s, bool coarse, bool enabled) : st(s), name(kernel) {
    if (!enabled || g_prof_mode != (coarse ? 2 : 1)) return;
    if (hipEventCreate(&start) != hipSuccess) {
        start = nullptr;
        return;
    }
    (void)hipEventRecord(start, st);
}
ProfScope::~ProfScope() {
    if (!start) return;
    hipEvent_t stop;
    if (hipEventCreate(&stop) != hipSuccess) {
        (void)hipEventDestroy(start);
        return;
    }
    (void)hipEventRecord(stop, st);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back({name, start, stop});
}
}  // namespace pcc

extern "C" {
void pcc_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(pcc::g_prof_mu);
    pcc::g_prof_mode = on;
    if (on) pcc::prof_clear();
}
void pcc_profile_reset(void) {
    std::lock_guard<std::mutex> lk(pcc::g_prof_mu);
    pcc::prof_clear();
}
int pcc_profile_read(const char *kernel_prefix, double *avg_us, int *launches) {
    std::lock_guard<std::mutex> lk(pcc::g_prof_mu);
    const std::string pre = kernel_prefix ? kernel_prefix : "";
    double total_ms = 0;
    int n = 0;
    for (auto &r : pcc::g_prof) {
        if (std::string(r.name).compare(0, pre.size(), pre) != 0) continue;
        if (hipEventSynchronize(r.b) != hipSuccess) continue;
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
        total_ms += ms;
        n++;
    }
    if (avg_us) *avg_us = n ? total_ms * 1e3 / n : 0.0;
    if (launches) *launches = n;
    return n ? PCC_OK : PCC_EINVAL;
}
size_t pcc_profile_names(char *buf, size_t capacity) {
    std::lock_guard<std::mutex> lk(pcc::g_prof_mu);
    std::vector<std::pair<std::string, int>> counts;  // in the order of each name's first launch
    for (auto &r : pcc::g_prof) {
        (void)hipEventSynchronize(r.b);
        auto it = counts.begin();
        while (it != counts.end() && it->first != r.name) ++it;
        if (it == counts.end()) counts.emplace_back(r.name, 1);
        else it->second++;
    }
    std::string text;
    for (auto &c : counts) text += c.first + '\t' + std::to_string(c.second) + '\n';
    if (buf && capacity) {
        const size_t len = text.size() < capacity - 1 ? text.size() : capacity - 1;
        std::memcpy(buf, text.data(), len);
        buf[len] = '\0';
    }
    return text.size() + 1;
}

const char *pcc_version(void) { return "pcc_structural 0.1 (gfx950)"; }
const char *pcc_last_error(void) { return t_msg; }
int pcc_last_status(void) { return t_status; }
}

namespace pcc {
bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    return cap != hipStreamCaptureStatusNone;
}

// per device: the sticky failure words [kind] (mapped host memory), the event of the last co-resident launch and its
// stream, pending test injections [kind]; guarded by g_coresident_mu
struct CoresidentDevice {
    unsigned *host = nullptr, *mapped = nullptr;
    hipEvent_t last = nullptr;
    hipStream_t last_stream = nullptr;
    bool inject[kCoresidentKinds] = {}, tried = false;
};
namespace {
std::mutex g_coresident_mu;
CoresidentDevice *coresident_device() {  // null if the state cannot be set up
    static CoresidentDevice devs[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    CoresidentDevice &d = devs[dev];
    if (!std::exchange(d.tried, true)) {
        void *h = nullptr, *p = nullptr;
        if (hipHostMalloc(&h, kCoresidentKinds * sizeof(unsigned), hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer(&p, h, 0) == hipSuccess && hipEventCreateWithFlags(&d.last, hipEventDisableTiming) == hipSuccess) {
            d.host = static_cast<unsigned *>(std::memset(h, 0, kCoresidentKinds * sizeof(unsigned)));
            d.mapped = static_cast<unsigned *>(p);
        } else {
            (void)hipGetLastError();
        }
    }
    return d.host ? &d : nullptr;
}
}  // namespace

CoresidentGate::CoresidentGate(CoresidentKind kind, hipStream_t s) : st(s) {
    if (capturing(st)) return;  // (first: nothing is set up, waited on or recorded inside a capture)
    g_coresident_mu.lock();
    if (!(dev = coresident_device())) {
        g_coresident_mu.unlock();
        return;
    }
    if (dev->last_stream && dev->last_stream != st) (void)hipStreamWaitEvent(st, dev->last, 0);
    ok = true;
    sticky = dev->mapped + kind;
    inject = std::exchange(dev->inject[kind], false);
}
CoresidentGate::~CoresidentGate() {
    if (!dev) return;
    if (hipEventRecord(dev->last, st) == hipSuccess) dev->last_stream = st;
    g_coresident_mu.unlock();
}

unsigned take_coresident_failure(CoresidentKind kind) {
    std::lock_guard<std::mutex> lk(g_coresident_mu);
    CoresidentDevice *d = coresident_device();
    return d ? __atomic_exchange_n(&d->host[kind], 0u, __ATOMIC_RELAXED) : 0;
}
}  // namespace pcc

// include/pcc_test_hooks.h: inert unless PCC_TEST_HOOKS=1 was in the environment when the library first looked
#include "pcc_test_hooks.h"
static bool hooks_armed() {
    static const bool armed = [] {
        const char *e = std::getenv("PCC_TEST_HOOKS");
        return e && e[0] == '1';
    }();
    return armed;
}
extern "C" int pcc_test_set_tuning(int key, int value) {
    if (!hooks_armed() || key < 0 || key >= PCC_TUNE_KEYS) return 0;
    __atomic_store_n(&g_tuning[key], value, __ATOMIC_RELAXED);
    return 1;
}
static int inject_failure(pcc::CoresidentKind kind) {
    if (!hooks_armed()) return 0;
    std::lock_guard<std::mutex> lk(pcc::g_coresident_mu);
    pcc::CoresidentDevice *d = pcc::coresident_device();
    if (d) d->inject[kind] = true;
    return d ? 1 : 0;
}
extern "C" int pcc_test_inject_auction_failure(void) { return inject_failure(pcc::kAuctionCluster); }
extern "C" int pcc_test_inject_approxmatch_failure(void) { return inject_failure(pcc::kFineResident); }
