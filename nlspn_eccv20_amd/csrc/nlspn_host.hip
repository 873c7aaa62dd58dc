// The library's shared host state (one per library, see nlspn_host.h): the error text,
// the per-device resident state, the A/B switches and the launch helper.
// No kernel is instantiated here.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "nlspn_host.h"

namespace nlspn {

namespace {
thread_local std::string g_err;
constexpr int kMaxDevices = 64;
DevState g_dev[kMaxDevices];
}  // namespace

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// ---------------------------------------------------------------- launches
int launch_kernel(const void *fn, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t s, const char *what,
                  hipEvent_t e0, hipEvent_t e1) {
    if (e0 || e1)
        NLSPN_HIP_TRY(hipExtLaunchKernel(fn, grid, block, args, lds, s, e0, e1, 0));
    else
        NLSPN_HIP_TRY(hipLaunchKernel(fn, grid, block, args, lds, s));
    return check_launch(what);
}

// ---------------------------------------------------------------- A/B switches
bool env_is(const char *name, char c) {
    const char *e = getenv(name);
    return e && e[0] == c;
}

unsigned env_dbg(const char *name, int base) {
    const char *e = kExperiments ? getenv(name) : nullptr;
    return e ? (unsigned)strtoul(e, nullptr, base) : 0u;
}

Switches read_switches() {
    Switches sw;
    sw.resident = !env_is("NLSPN_RESIDENT", '0');
    sw.res_first = !env_is("NLSPN_RES_FIRST", '0');
    sw.res_split = env_is("NLSPN_RES_SPLIT", '0') ? 0 : env_is("NLSPN_RES_SPLIT", '2') ? 2 : 1;
    sw.res_merge = !env_is("NLSPN_RES_MERGE", '0');
    sw.res_l2 = !env_is("NLSPN_RES_L2", '0');
    sw.res_offcopy = !env_is("NLSPN_RES_OFFCOPY", '0');
    sw.res_helper = !env_is("NLSPN_RES_HELPER", '0');
    if (const char *gs = getenv("NLSPN_RES_GRID"))  // "gy,gx" or "gyxgx"
        if (sscanf(gs, "%d%*c%d", &sw.res_gy, &sw.res_gx) != 2) sw.res_gy = sw.res_gx = 0;
    sw.res_dbg = env_dbg("NLSPN_RES_DBG");
    return sw;
}

// ---------------------------------------------------------------- per-device state
int device_cus() {
    static int cached[kMaxDevices] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cached[dev] = n;
    }
    return cached[dev];
}

DevState *dev_state() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
    DevState &d = g_dev[dev];
    std::lock_guard<std::mutex> lk(d.m);
    if (!d.init) {
        void *h = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
            void *dp = nullptr;
            if (hipHostGetDevicePointer(&dp, h, 0) == hipSuccess) {
                d.host_status = static_cast<unsigned *>(h);
                d.dev_status = static_cast<unsigned *>(dp);
                *d.host_status = 0u;
            } else {
                (void)hipHostFree(h);
            }
        }
        d.init = true;
    }
    return &d;
}

int set_lds_attr(const void *fn, int lds) {
    DevState *d = dev_state();
    if (d) {
        std::lock_guard<std::mutex> lk(d->m);
        for (const auto &e : d->lds_attr)
            if (e.first == fn && e.second >= lds) return NLSPN_OK;
    }
    NLSPN_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if (d) {
        std::lock_guard<std::mutex> lk(d->m);
        d->lds_attr.emplace_back(fn, lds);
    }
    return NLSPN_OK;
}

namespace {
bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

bool res_guard_off() {  // A/B measurement only, experiments build: NLSPN_RES_GUARD=0 (read once)
    if (!kExperiments) return false;
    static const bool off = [] { const char *e = getenv("NLSPN_RES_GUARD"); return e && e[0] == '0'; }();
    return off;
}
}  // namespace

int res_guard_before(hipStream_t s) {
    if (res_guard_off() || stream_capturing(s)) return NLSPN_OK;
    DevState *d = dev_state();
    if (!d) return NLSPN_OK;
    std::lock_guard<std::mutex> lk(d->m);
    if (d->any && d->last_stream != s) {
        if (!d->multi) {  // first switch: everything earlier finishes, then record per launch
            NLSPN_HIP_TRY(hipDeviceSynchronize());
            d->multi = true;
        } else if (d->last_ev) {
            NLSPN_HIP_TRY(hipStreamWaitEvent(s, d->last_ev, 0));
        }
    }
    return NLSPN_OK;
}

int res_guard_after(hipStream_t s) {
    if (res_guard_off() || stream_capturing(s)) return NLSPN_OK;
    DevState *d = dev_state();
    if (!d) return NLSPN_OK;
    std::lock_guard<std::mutex> lk(d->m);
    d->any = true;
    d->last_stream = s;
    if (!d->multi) return NLSPN_OK;
    if (!d->last_ev) NLSPN_HIP_TRY(hipEventCreateWithFlags(&d->last_ev, hipEventDisableTiming));
    NLSPN_HIP_TRY(hipEventRecord(d->last_ev, s));
    return NLSPN_OK;
}

}  // namespace nlspn

extern "C" {

int nlspn_abi_version(void) { return NLSPN_ABI_VERSION; }

const char *nlspn_last_error(void) { return nlspn::g_err.c_str(); }

}  // extern "C"
