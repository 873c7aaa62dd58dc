// Host side shared by the C-ABI translation units (nlspn_prop_fwd.hip, nlspn_prop_bwd.hip,
// nlspn_seam.hip, nlspn_gconv_host.hip): the error state behind nlspn_last_error, argument
// validators, the launch and event-timing helpers, the per-device state of the resident
// kernels and the A/B switches.  The state is one per library: it is defined in
// nlspn_host.hip, never in this header.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <mutex>
#include <utility>
#include <vector>

#include "../../include/nlspn_prop.h"
#include "nlspn_common.h"
#include "nlspn_plan.h"

namespace nlspn {
#pragma GCC visibility push(hidden)  // host helpers: not part of the library's exported symbols

// Sets the calling thread's error text (nlspn_last_error) and returns code.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define NLSPN_HIP_TRY(expr)                                                               \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail(NLSPN_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// returns a failed step's code (a validator's, a launch's)
#define NLSPN_TRY(expr)                \
    do {                               \
        if (int rc_ = (expr)) return rc_; \
    } while (0)

inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(NLSPN_EHIP, "error in %s: %s", what, hipGetErrorString(e));
    return NLSPN_OK;
}

inline size_t esize(int dtype) { return dtype == NLSPN_DTYPE_F16 ? 2 : 4; }

inline bool aligned(const void *p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline unsigned elementwise_grid(long long groups) {
    long long g = (groups + 255) / 256;
    if (g > 256 * 16) g = 256 * 16;
    return (unsigned)(g < 1 ? 1 : g);
}

// ---- argument validators: NLSPN_OK, or the code with the message set
inline int check_storage_dtype(int dtype) {  // f32 or f16 storage
    return dtype == NLSPN_DTYPE_F32 || dtype == NLSPN_DTYPE_F16
               ? NLSPN_OK : fail(NLSPN_EUNSUPPORTED, "dtype %d not supported (f32=0, f16=1)", dtype);
}
inline int check_f32(int dtype, const char *what) {
    return dtype == NLSPN_DTYPE_F32 ? NLSPN_OK : fail(NLSPN_EUNSUPPORTED, "%s: float32 only (dtype %d)", what, dtype);
}
inline int check_nonempty(int B, int H, int W) {
    return B < 1 || H < 1 || W < 1 ? fail(NLSPN_EINVAL, "empty input: B=%d H=%d W=%d", B, H, W) : NLSPN_OK;
}
inline int check_odd_kernel(int kh, int kw) {
    return kh < 1 || kw < 1 || (kh % 2) == 0 || (kw % 2) == 0 || kh * kw < 2
               ? fail(NLSPN_EINVAL, "only odd kernel is supported but k = %dx%d", kh, kw) : NLSPN_OK;
}
inline int check_prop_time(int T) { return T < 1 ? fail(NLSPN_EINVAL, "prop_time must be >= 1, got %d", T) : NLSPN_OK; }
inline int check_kind(int kind) {
    return kind < NLSPN_AFF_AS || kind > NLSPN_AFF_TGASS ? fail(NLSPN_EINVAL, "unknown affinity kind %d", kind) : NLSPN_OK;
}
inline int check_preserve(unsigned flags, const void *dep) {
    return (flags & NLSPN_PRESERVE_INPUT) && !dep ? fail(NLSPN_EINVAL, "preserve_input requires dep") : NLSPN_OK;
}
// a batch stride of at least `planes` H*W planes; what: "aff" or "offset"
inline int check_batch_stride(const char *what, long long bs, long long planes, long long HW) {
    return bs < planes * HW ? fail(NLSPN_EINVAL, "%s batch stride %lld < %lld*H*W", what, bs, planes) : NLSPN_OK;
}
// one batch item's 3K + 4 planes stay below 2 GiB (32-bit buffer offsets into an item)
inline int check_item_bytes(long long HW, int K, size_t es) {
    return HW * (3LL * K + 4) * (long long)es > 0x7fffffffLL
               ? fail(NLSPN_EINVAL, "image too large: one batch item's planes must stay below 2 GiB") : NLSPN_OK;
}

// One kernel launch and its error check; with e0 / e1 the dispatch-recorded event pair
// around it (hipExtLaunchKernel).
int launch_kernel(const void *fn, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t s, const char *what,
                  hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// Timing events of the nlspn_time_* entry points, destroyed with the object.
struct TimingEvents {
    std::vector<hipEvent_t> ev;
    explicit TimingEvents(size_t n) : ev(n, nullptr) {}
    ~TimingEvents() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create() {
        for (hipEvent_t &e : ev) NLSPN_HIP_TRY(hipEventCreate(&e));
        return NLSPN_OK;
    }
    int elapsed(size_t first, float *ms) {  // between ev[first] and ev[first + 1]
        NLSPN_HIP_TRY(hipEventElapsedTime(ms, ev[first], ev[first + 1]));
        return NLSPN_OK;
    }
};

int device_cus();  // CUs of the current device (cached), 0 without one

// The A/B switches of the environment, read on every call: the forward resident path's
// (nlspn_plan.h Switches); one switch, whether its value starts with c; a NLSPN_*_DBG word
// (0 outside the experiments build)
Switches read_switches();
bool env_is(const char *name, char c);
unsigned env_dbg(const char *name, int base = 10);

// Per-device state of the resident path.
//  * status: a host-mapped sticky word the resident kernel sets when a launch
//    aborts (nlspn_resident.h); nlspn_resident_status reads it with no device sync.
//  * res_guard: the resident kernel needs every workgroup co-resident, so two of
//    its launches must never run at once on one device.  Resident launches are
//    serialised across streams.  While one stream issues them all (the common case)
//    nothing is recorded: an event record per launch costs ~3 us of stream time
//    (measured, C2).  The first resident launch on a second stream synchronises the
//    device once (no handle of the earlier stream is touched: it may be gone) and
//    switches the device to multi-stream mode, where every resident launch records
//    an event and a launch on another stream waits for the previous one's event.
//    (Skipped while a stream is being captured: a plan re-applies the guard when it
//    is launched.)
struct DevState {
    std::mutex m;
    unsigned *host_status = nullptr, *dev_status = nullptr;
    hipEvent_t last_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool any = false, multi = false;
    bool init = false;
    std::vector<std::pair<const void *, int>> lds_attr;  // kernels whose LDS limit is raised (set_lds_attr)
};
DevState *dev_state();

// Raises a kernel's dynamic-LDS limit once per (device, kernel, size): the attribute is
// per device, and launches come from several threads and devices, so it is checked on
// every launch, but the driver call is made only the first time.
int set_lds_attr(const void *fn, int lds);

// around every resident launch (forward and backward), see DevState
int res_guard_before(hipStream_t s);
int res_guard_after(hipStream_t s);

#pragma GCC visibility pop
}  // namespace nlspn
