// C ABI of the forward propagation (see include/nlspn_prop.h): step dispatch, the resident
// plan's arguments and launches, the T-iteration launch sequence, hipGraph plans and the
// dispatch-event timing entry points used by bench.py.  The step kernels are instantiated
// here; the resident kernels in nlspn_kern_resident.hip / nlspn_kern_resident_wide.hip.
#include <vector>

#include "nlspn_host.h"
#include "nlspn_resident.h"
#include "nlspn_step.h"

namespace nlspn {
// defined in nlspn_kern_resident.hip and nlspn_kern_resident_wide.hip (own translation units)
NLSPN_RES_BUILDS_3X3(NLSPN_RES_EXTERN)
NLSPN_RES_BUILDS_WIDE(NLSPN_RES_EXTERN)
NLSPN_RES_NOCOPY_3X3(NLSPN_RES_EXTERN_NOCOPY)
NLSPN_RES_NOCOPY_WIDE(NLSPN_RES_EXTERN_NOCOPY)
}  // namespace nlspn

using namespace nlspn;

namespace {

// ---------------------------------------------------------------- step dispatch
struct StepLaunch {
    const void *fn = nullptr;  // kernel address
    dim3 grid, block;
};

template <typename T, int KH, int KW, int TH, int TW, int PX, int RY, int RX, int SV, bool OFFSET, bool PRE>
StepLaunch make_step(StepArgs &a, bool first) {
    StepLaunch L;
    L.fn = first ? reinterpret_cast<const void *>(&prop_step_kernel<T, KH, KW, TH, TW, PX, RY, RX, SV, OFFSET, PRE, true>)
                 : reinterpret_cast<const void *>(&prop_step_kernel<T, KH, KW, TH, TW, PX, RY, RX, SV, OFFSET, PRE, false>);
    a.tiles_x = (a.W + TW - 1) / TW;
    a.tiles_y = (a.H + TH - 1) / TH;
    L.grid = dim3((unsigned)(a.B * a.tiles_x * a.tiles_y));
    L.block = dim3(TH * TW / PX);
    return L;
}

// Tile configurations per geometry.  vec: 16-B staging loads, needs W % 4 == 0
// and aligned planes; scalar: any shape.  Tiles measured with tools/step_bench
// (interleaved A/B, dispatch events): one pixel per lane and small 8x32 tiles
// keep the kernel at the streaming ceiling of its 4+3K planes.
template <typename T>
int select_step(StepArgs &a, int kh, int kw, bool offset, bool vec, bool first, StepLaunch &L) {
    if (!offset) {
        if (kh != 3 || kw != 3)
            return fail(NLSPN_EUNSUPPORTED,
                        "no-offset propagation is 3x3 replicate (nlspnmodel.py:209-224); got %dx%d", kh, kw);
        L = vec ? make_step<T, 3, 3, 16, 64, 4, 1, 1, 1, false, true>(a, first)
                : make_step<T, 3, 3, 4, 64, 1, 1, 1, 1, false, true>(a, first);
        return NLSPN_OK;
    }
    // 1x17: a 10-row / 20-column halo (12 columns beyond the widest base tap) keeps the
    // global fallback off all but ~1e-6 of the pixels at N(0, 2^2) offsets: 24.3 vs 24.6 us
    // per C5 step against the 8 / 16 halo (profiles/r03/ab_*_halo_v1.txt); for 3x3 the
    // wider window (12 / 12) measured within noise (C2 +0.2 %, C3 -0.7 %) and is not used.
    if (kh == 3 && kw == 3)
        L = vec ? make_step<T, 3, 3, 8, 32, 1, 8, 8, 4, true, true>(a, first)
                : make_step<T, 3, 3, 4, 64, 1, 8, 8, 1, true, true>(a, first);
    else if (kh == 1 && kw == 17)
        L = vec ? make_step<T, 1, 17, 8, 32, 1, 10, 20, 4, true, true>(a, first)
                : make_step<T, 1, 17, 4, 64, 1, 8, 16, 1, true, true>(a, first);
    else if (kh == 5 && kw == 5)
        L = vec ? make_step<T, 5, 5, 8, 32, 1, 8, 8, 4, true, true>(a, first)
                : make_step<T, 5, 5, 4, 64, 1, 8, 8, 1, true, true>(a, first);
    else if (kh == 7 && kw == 7)
        L = vec ? make_step<T, 7, 7, 8, 32, 1, 8, 8, 4, true, true>(a, first)
                : make_step<T, 7, 7, 4, 64, 1, 8, 8, 1, true, true>(a, first);
    else
        return fail(NLSPN_EUNSUPPORTED, "no kernel instantiation for a %dx%d propagation geometry "
                    "(supported: 3x3, 5x5, 7x7, 1x17)", kh, kw);
    return NLSPN_OK;
}

struct StepReq {
    int dtype;
    StepArgs a;
    int kh, kw;
    bool first = false;  // fused-prologue first iteration
};

int prepare_step(StepReq &r, StepLaunch &L) {
    StepArgs &a = r.a;
    NLSPN_TRY(check_storage_dtype(r.dtype));
    NLSPN_TRY(check_nonempty(a.B, a.H, a.W));
    NLSPN_TRY(check_odd_kernel(r.kh, r.kw));
    if (!a.p_in || !a.aff || !a.p_out) return fail(NLSPN_EINVAL, "p_in, aff and p_out must be non-null");
    NLSPN_TRY(check_preserve(a.flags, a.dep));
    const long long HW = (long long)a.H * a.W;
    const int K = r.kh * r.kw - 1;
    NLSPN_TRY(check_batch_stride("aff", a.aff_bs, r.first ? K : K + 1, HW));
    NLSPN_TRY(check_item_bytes(HW, K, esize(r.dtype)));
    if (a.off) NLSPN_TRY(check_batch_stride("offset", a.off_bs, a.off_raw ? 2 * K : 2 * (K + 1), HW));
    if ((long long)a.B * ((a.H + 3) / 4) * ((a.W + 63) / 64) > 0x7fffffffLL)
        return fail(NLSPN_EINVAL, "grid too large");
    const size_t vb = 4 * esize(r.dtype);
    // Element-aligned planes suffice for the 1-pixel-per-lane loads; 16-B window
    // staging needs W % 4 == 0 and a 16-B aligned p_in / conf / dep.
    const bool vec = (a.W % 4 == 0) && aligned(a.p_in, vb) && aligned(a.conf, vb) && aligned(a.dep, vb);
    return r.dtype == NLSPN_DTYPE_F32 ? select_step<float>(a, r.kh, r.kw, a.off != nullptr, vec, r.first, L)
                                      : select_step<__half>(a, r.kh, r.kw, a.off != nullptr, vec, r.first, L);
}

// ---------------------------------------------------------------- launches
// A plan's launch record: enough to re-issue one kernel launch without a graph.
struct LaunchRec {
    const void *fn;
    dim3 grid, block;
    size_t lds;
    bool resident;
    StepArgs sa;
    ResArgs ra;
};
thread_local std::vector<LaunchRec> *g_rec = nullptr;  // set while nlspn_plan_create records

// One launch of the section (a step's or a resident one), with its optional dispatch events;
// recorded while a plan is being created.
int launch_section(const LaunchRec &r, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (g_rec) g_rec->push_back(r);
    void *args[] = {const_cast<void *>(r.resident ? static_cast<const void *>(&r.ra) : static_cast<const void *>(&r.sa))};
    if (!r.resident) return launch_kernel(r.fn, r.grid, r.block, args, 0, s, "nlspn_prop_step", e0, e1);
    NLSPN_TRY(res_guard_before(s));
    NLSPN_TRY(launch_kernel(r.fn, r.grid, r.block, args, r.lds, s, "nlspn_propagate resident", e0, e1));
    return res_guard_after(s);
}

int launch(const StepLaunch &L, const StepArgs &a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
    return launch_section(LaunchRec{L.fn, L.grid, L.block, 0, false, a, ResArgs{}}, s, e0, e1);
}

// ------------------------------------------------------------ resident dispatch
// Iterations 2..T in one launch with the invariant planes held on chip
// (nlspn_resident.h).  Applies to the 3x3, 1x17 and 5x5 learned-offset geometries when
// every part's quads fit one workgroup and its window fits LDS; otherwise the T-1
// per-iteration launches run.  The decisions are nlspn_plan.h res_plan's; this unit maps
// its record to kernel addresses and arguments.

// What a section gives the resident launches besides its shape.
struct ResInputs {
    int dtype;
    const void *conf_eff, *dep, *aff_norm, *off_raw;
    long long off_bs;
    void *pred_inter, *pred, *workspace;
    unsigned flags;
    void *off_out = nullptr;
    // The prologue's inputs and outputs, for a plan that runs it inside the launch (kResFirst:
    // then no step-1 launch precedes the resident launches); has_first false: step 1 runs
    bool has_first = false;
    const void *pinit = nullptr, *conf_raw = nullptr, *aff_raw = nullptr;
    long long aff_bs = 0;
    const float *gamma = nullptr;
    int kind = 0;
    void *aff_out = nullptr, *conf_out = nullptr;  // conf_out null iff conf_raw null
};

struct ResPlan {
    ResPlanRec rec;
    const void *fn = nullptr;
    const void *fn_merged = nullptr;  // launch 0's kernel when it runs several image groups
    // the same builds without the loop's copy code (prop_resident_kernel COPY = false), for the
    // launches whose main waves copy nothing (ResArgs::off_out null); null: the build has one form
    const void *fn_nc = nullptr, *fn_merged_nc = nullptr;
    int nlaunch = 0;
    int err = 0;  // nonzero: the plan was refused with an error (not a fallback), see nlspn_last_error
    ResArgs a[kResMaxGroups];
};

// the kernel of a plan's launches (groups: the merged launch 0's), null: no such build;
// nocopy: its form without the loop's copy code (null: the build copies in its setup)
template <typename T>
const void *res_kernel(const ResPlanRec &R, bool groups, bool nocopy = false) {
    const int ntc = groups ? R.ntc_merged : R.ntc;
    if (nocopy) {
#define NLSPN_RES_LOOKUP(KH, KW, NTC, G, F)                                  \
    if (R.kh == KH && ntc == NTC && groups == G && R.first == F && R.split == 0) \
        return reinterpret_cast<const void *>(&prop_resident_kernel<T, KH, KW, kResMaxNT, kResSMax, NTC, G, F, 0, false>);
        NLSPN_RES_NOCOPY_3X3(NLSPN_RES_LOOKUP)
        NLSPN_RES_NOCOPY_WIDE(NLSPN_RES_LOOKUP)
#undef NLSPN_RES_LOOKUP
        return nullptr;
    }
#define NLSPN_RES_LOOKUP(KH, KW, NTC, G, F, PXO)                                  \
    if (R.kh == KH && ntc == NTC && groups == G && R.first == F && R.split == PXO) \
        return reinterpret_cast<const void *>(&prop_resident_kernel<T, KH, KW, kResMaxNT, kResSMax, NTC, G, F, PXO>);
    NLSPN_RES_BUILDS_3X3(NLSPN_RES_LOOKUP)
    NLSPN_RES_BUILDS_WIDE(NLSPN_RES_LOOKUP)
#undef NLSPN_RES_LOOKUP
    return nullptr;
}

// What res_plan needs to know of the pointers: all given and 16-B aligned; and whether the
// prologue can run in the launch (raw inputs and prologue outputs 16-B aligned, raw offset
// layout; NLSPN_RES_FIRST=0 (A/B) keeps step 1 in front)
void res_query(const ResInputs &in, const Switches &sw, ResPlanRec &R) {
    const size_t vb = 4 * (size_t)R.es;
    R.ptrs_ok = in.workspace && in.off_raw && aligned(in.conf_eff, vb) && aligned(in.dep, vb) &&
                         aligned(in.aff_norm, vb) && aligned(in.off_raw, vb) && aligned(in.pred_inter, vb) &&
                         aligned(in.pred, vb) && in.off_bs % 4 == 0 && aligned(in.workspace, 16);
    R.first_ok = in.has_first && sw.res_first && aligned(in.pinit, vb) && aligned(in.conf_raw, vb) &&
                          aligned(in.aff_raw, vb) && aligned(in.aff_out, vb) && aligned(in.conf_out, vb) &&
                          aligned(in.off_out, vb) && in.aff_bs % 4 == 0 && in.gamma && in.aff_out &&
                  !(in.flags & kResOffInserted);
}

// where a resident launch copies the inserted offsets to (its main waves or its helper wave), or null
void *res_off_dst(const ResArgs &a) { return a.off_out ? a.off_out : a.off_out_h; }

// Step 3 of the plan, the arguments: ResArgs per image group, then the merged launch.
void res_fill_args(const ResInputs &in, int B, int H, int W, int K, int T, const Switches &sw, ResPlan &P) {
    const ResPlanRec &R = P.rec;
    const ResShape &S = R.S;
    const size_t es = esize(in.dtype), vb = 4 * es;
    const long long HW = (long long)H * W;
    DevState *ds = dev_state();
    // Per-line hand-offs (kResL2, nlspn_resident.h: a 128-B line no part on another XCC reads
    // is stored plain and stays in its XCD's L2): possible where every image plane of every
    // iteration starts and ends on a 128-B line (no line is shared by two images) and an
    // image row holds at least a line (a line then spans at most two rows); NLSPN_RES_L2=0
    // (A/B) exports every line (write-through)
    const bool l2ok = sw.res_l2 && ((long long)HW * (long long)es) % 128 == 0 && aligned(in.pred_inter, 128) &&
                      ((long long)B * HW * (long long)es) % 128 == 0 && (long long)(W / 4) * 4 * (long long)es >= 128 &&
                      H < 65536 && W / 4 < 65536;
    // the output dict's inserted offsets copied by the resident loop (ResArgs::off_out)
    // instead of step 1; NLSPN_RES_OFFCOPY=0 (A/B) leaves them to step 1
    const bool copy_off = in.off_out && ((!(in.flags & kResOffInserted) && sw.res_offcopy && aligned(in.off_out, vb)) || R.first);
    // ... by a helper wave (kResHelper: the launch has S.nt + 64 threads) in the builds that copy
    // in the loop (ntc: the build's compile-time thread count; the 128-thread and split-quad
    // builds copy in their setup), where the launch bound has room for the wave;
    // NLSPN_RES_HELPER=0 (A/B) keeps the main waves' copy
    const auto helper = [&](int ntc) {
        return copy_off && sw.res_helper && ntc != 128 && !R.split && S.nt % 64 == 0 && S.nt + 64 <= kResMaxNT;
    };
    // the destination goes to the copying waves' field: off_out (the main waves') or off_out_h
    // (the helper's, with the flag); the other stays null
    const auto set_copy = [&](ResArgs &a, void *dst, int ntc) {
        const bool h = helper(ntc);
        a.flags = (a.flags & ~kResHelper) | (h ? kResHelper : 0u);
        a.off_out = h ? nullptr : dst;
        a.off_out_h = h ? dst : nullptr;
    };
    for (int k = 0; k < R.ngroups; ++k) {
        const long long b0 = (long long)k * S.Bg;
        auto at = [&](const void *p, long long elems) -> const void * {
            return p ? static_cast<const char *>(p) + (size_t)(elems * (long long)es) : nullptr;
        };
        // progress values of group k: epoch + 1 .. epoch + T, epoch = k (T + 1)
        P.a[k] = ResArgs{at(in.conf_eff, b0 * HW), (in.flags & kPreserve) ? at(in.dep, b0 * HW) : nullptr,
                         at(in.aff_norm, b0 * (K + 1) * HW), at(in.off_raw, b0 * in.off_bs),
                         const_cast<void *>(at(in.pred_inter, b0 * HW)), const_cast<void *>(at(in.pred, b0 * HW)),
                         static_cast<unsigned *>(in.workspace), ds ? ds->dev_status : nullptr, in.off_bs,
                         (long long)B * HW, (int)std::min<long long>(S.Bg, B - b0), H, W, T, S.gy, S.gx, S.win_cells,
                         (unsigned)(k * (T + 1)), in.flags | (l2ok ? kResL2 : 0u), sw.res_dbg};
        if (copy_off) set_copy(P.a[k], const_cast<void *>(at(in.off_out, b0 * 2 * (K + 1) * HW)), R.ntc);
        if (R.first) {  // the prologue in the launch: raw inputs, conf' written here (read back by the rim staging)
            P.a[k].flags |= kResFirst;
            P.a[k].conf = at(in.conf_out, b0 * HW);
            P.a[k].aff = at(in.aff_raw, b0 * in.aff_bs);
            P.a[k].aff_bs = in.aff_bs;
            P.a[k].pinit = at(in.pinit, b0 * HW);
            P.a[k].conf_raw = at(in.conf_raw, b0 * HW);
            P.a[k].gamma = in.gamma;
            P.a[k].kind = in.kind;
            P.a[k].aff_out = const_cast<void *>(at(in.aff_out, b0 * (K + 1) * HW));
        }
    }
    P.nlaunch = R.ngroups;
    // (every merged shape has a GROUPS build; should one be missing, the groups launch
    // one by one rather than a single-group build running only group 0)
    if (!R.merged || !P.fn_merged) return;
    P.nlaunch = 1;
    if (R.ngroups > R.nfull) P.a[P.nlaunch++] = P.a[R.ngroups - 1];  // the partial group, launched after the merged one
    P.a[0].ngroups = R.nfull;
    if (copy_off) set_copy(P.a[0], res_off_dst(P.a[0]), R.ntc_merged);  // (the merged launch's build)
}

// Fills P and returns true when the resident kernel applies (iterations 2..T).
bool plan_resident(const ResInputs &in, int B, int H, int W, int kh, int kw, int T, ResPlan &P) {
    const Switches sw = read_switches();
    const bool f32 = in.dtype == NLSPN_DTYPE_F32;
    ResPlanRec &R = P.rec;
    R.es = (int)esize(in.dtype);
    R.B = B; R.H = H; R.W = W; R.kh = kh; R.kw = kw; R.T = T;
    res_query(in, sw, R);
    if (!res_plan(device_cus(), sw, R)) return false;
    P.fn = f32 ? res_kernel<float>(R, false) : res_kernel<__half>(R, false);
    if (!P.fn) return false;
    P.fn_nc = f32 ? res_kernel<float>(R, false, true) : res_kernel<__half>(R, false, true);
    if (sw.res_dbg & 8u) {  // trace stamps (experiments build) go into pred: each launch's part must hold them
        const long long HW = (long long)H * W;
        const long long per = (long long)(T + 1) * (kResWTrace ? 29 : 5) * 8;  // rows: the setup, then one per iteration
        for (int k = 0; k < R.ngroups; ++k) {
            const long long room = (long long)(B - (long long)k * R.S.Bg) * HW * (long long)R.es;
            if (room < (long long)R.grid[k] * per) {
                P.err = fail(NLSPN_EINVAL, "resident trace (NLSPN_RES_DBG=8): pred holds %lld bytes from image group %d, "
                             "the stamps need %lld", room, k, (long long)R.grid[k] * per);
                return false;
            }
        }
    }
    // the group-loop build for the merged launch; a partial last group keeps the other
    if (R.merged) P.fn_merged = f32 ? res_kernel<float>(R, true) : res_kernel<__half>(R, true);
    if (R.merged) P.fn_merged_nc = f32 ? res_kernel<float>(R, true, true) : res_kernel<__half>(R, true, true);
    res_fill_args(in, B, H, W, kh * kw - 1, T, sw, P);
    return true;
}

// The sync words must be zero on entry and plane 1 poisoned (T >= 3): step 1 does both
// (arm_resident).
// e0 is recorded at the start of the first group's launch, e1 at the end of the last.
int launch_resident(ResPlan &P, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
    NLSPN_TRY(set_lds_attr(P.fn, (int)P.rec.lds));
    if (P.fn_merged) NLSPN_TRY(set_lds_attr(P.fn_merged, (int)P.rec.lds));
    if (P.fn_nc) NLSPN_TRY(set_lds_attr(P.fn_nc, (int)P.rec.lds));
    if (P.fn_merged_nc) NLSPN_TRY(set_lds_attr(P.fn_merged_nc, (int)P.rec.lds));
    if (P.a[0].ngroups > 1 && !P.fn_merged)  // (plan_resident never makes one: a single-group build would run group 0 only)
        return fail(NLSPN_EINVAL, "resident plan: %d merged image groups without a group-loop build", P.a[0].ngroups);
    for (int k = 0; k < P.nlaunch; ++k) {
        const bool mg = k == 0 && P.fn_merged;
        const void *fn = mg ? P.fn_merged : P.fn;
        // main waves that copy nothing run the build without the copy code
        const void *nc = mg ? P.fn_merged_nc : P.fn_nc;
        if (!P.a[k].off_out && nc) fn = nc;
        const unsigned grid = (unsigned)(P.a[k].B * P.a[k].gy * P.a[k].gx);  // a part per workgroup
        // (kResHelper: the helper wave behind the S.nt quad-owning threads)
        const unsigned block = (unsigned)P.rec.S.nt + ((P.a[k].flags & kResHelper) ? 64u : 0u);
        NLSPN_TRY(launch_section(LaunchRec{fn, dim3(grid), dim3(block), P.rec.lds, true, StepArgs{}, P.a[k]},
                                 s, k == 0 ? e0 : nullptr, k == P.nlaunch - 1 ? e1 : nullptr));
    }
    return NLSPN_OK;
}

// Step 1 in front of resident launches zeroes their sync words and poisons plane 1 (the
// hand-off's "not yet written" value, T >= 3): StepArgs::zero_words, ::nzero, ::poison.
void arm_resident(StepArgs &a1, const ResPlan &P, void *pred_inter, long long N, size_t es, int T) {
    a1.zero_words = P.a[0].sync;
    a1.nzero = (int)(P.rec.sync_bytes / 4);
    a1.poison = T >= 3 ? static_cast<char *>(pred_inter) + (size_t)N * es : nullptr;
}

// Iterations t_from + 1 .. T as step launches: list_pred[t] lands in pred_inter[t].  ev
// (optional): the dispatch-recorded pair [2t, 2t + 1] around iteration t + 1.
int run_steps(const StepLaunch &L, const StepArgs &base, void *pred_inter, void *pred, long long N, size_t es, int t_from,
              int T, hipStream_t s, hipEvent_t *ev) {
    for (int t = t_from; t < T; ++t) {
        StepArgs a = base;
        a.p_in = static_cast<const char *>(pred_inter) + (size_t)(t - 1) * N * es;
        a.p_out = static_cast<char *>(pred_inter) + (size_t)t * N * es;
        a.pred_out = t == T - 1 ? pred : nullptr;
        NLSPN_TRY(launch(L, a, s, ev ? ev[2 * t] : nullptr, ev ? ev[2 * t + 1] : nullptr));
    }
    return NLSPN_OK;
}

// The whole section (see nlspn_propagate).  ev (optional, 2*T events): a dispatch-
// recorded pair around each launch — [0,1] step 1 (an empty interval when the resident
// launches run the prologue), then [2,3] the resident kernel or [2t, 2t+1] per-iteration
// step t+1.  *resident (optional): the resident launches' count if the resident kernel
// ran iterations 2..T, | kResidentFirstBit if it also ran the prologue and iteration 1.
constexpr int kResidentFirstBit = 0x100;  // (bench.py RESIDENT_FIRST)
int propagate_impl(int dtype, const void *pred_init, const void *dep, const void *conf, const void *aff_raw,
                   int64_t aff_bstride, const void *off_raw, int64_t off_bstride, const float *gamma,
                   void *pred_inter, void *pred, void *aff_out, void *off_out, void *conf_out, void *workspace,
                   int B, int H, int W, int kh, int kw, int T, int kind, unsigned flags, hipStream_t s,
                   hipEvent_t *ev, int *resident) {
    NLSPN_TRY(check_storage_dtype(dtype));
    NLSPN_TRY(check_nonempty(B, H, W));
    NLSPN_TRY(check_prop_time(T));
    NLSPN_TRY(check_kind(kind));
    NLSPN_TRY(check_odd_kernel(kh, kw));
    if (!pred_init || !aff_raw || !gamma || !pred_inter || !pred || !aff_out)
        return fail(NLSPN_EINVAL, "null required pointer");
    NLSPN_TRY(check_preserve(flags, dep));
    if (conf && !conf_out) return fail(NLSPN_EINVAL, "conf given without conf_out");
    if (off_out && !off_raw) return fail(NLSPN_EINVAL, "off_out given without off_raw");
    const int K = kh * kw - 1;
    const long long HW = (long long)H * W, N = (long long)B * HW;
    NLSPN_TRY(check_batch_stride("aff", aff_bstride, K, HW));
    if (off_raw) NLSPN_TRY(check_batch_stride("offset", off_bstride, 2 * K, HW));
    const size_t es = esize(dtype);
    void *conf_eff = conf ? conf_out : nullptr;

    // iteration 1 with the prologue fused in (raw head outputs in, output-dict
    // tensors out), then T-1 steps on the normalised affinity and conf'
    StepReq r1{dtype, StepArgs{pred_init, conf, dep, aff_raw, off_raw, pred_inter, T == 1 ? pred : nullptr,
                               aff_bstride, off_bstride, B, H, W, 0, 0, 1, flags, gamma, aff_out, off_out,
                               conf_eff, kind},
               kh, kw, true};
    StepLaunch L1;
    NLSPN_TRY(prepare_step(r1, L1));
    StepReq r{dtype, StepArgs{pred_inter, conf_eff, dep, aff_out, off_raw, pred_inter, pred, (long long)(K + 1) * HW,
                              off_bstride, B, H, W, 0, 0, 1, flags, nullptr, nullptr, nullptr, nullptr, 0},
              kh, kw};
    StepLaunch L;
    if (T > 1) NLSPN_TRY(prepare_step(r, L));

    if (resident) *resident = 0;
    ResPlan P;
    // the prologue and iteration 1 inside the resident launches (no step-1 launch) where the
    // resident kernel applies (res_plan_first)
    ResInputs in{dtype, conf_eff, dep, aff_out, off_raw, off_bstride, pred_inter, pred, workspace, flags, off_out};
    in.has_first = true;
    in.pinit = pred_init; in.conf_raw = conf; in.aff_raw = aff_raw; in.aff_bs = aff_bstride;
    in.gamma = gamma; in.kind = kind; in.aff_out = aff_out; in.conf_out = conf_eff;
    const bool res = plan_resident(in, B, H, W, kh, kw, T, P);
    if (P.err) return P.err;
    if (res && P.rec.first) {
        // The resident kernel's sync words start every launch at zero and every launch leaves
        // them zero (res_finish); a plan clears its workspace once at creation, a direct call
        // clears it here (the caller's workspace may hold anything)
        if (!g_rec) NLSPN_HIP_TRY(hipMemsetAsync(workspace, 0, P.rec.sync_bytes, s));
        if (ev) {  // no step 1: an empty interval
            NLSPN_HIP_TRY(hipEventRecord(ev[0], s));
            NLSPN_HIP_TRY(hipEventRecord(ev[1], s));
        }
        if (resident) *resident = P.nlaunch | kResidentFirstBit;
        return launch_resident(P, s, ev ? ev[2] : nullptr, ev ? ev[3] : nullptr);
    }
    if (res && res_off_dst(P.a[0])) r1.a.off_out = nullptr;  // the resident loop copies the offsets
    if (res) arm_resident(r1.a, P, pred_inter, N, es, T);
    NLSPN_TRY(launch(L1, r1.a, s, ev ? ev[0] : nullptr, ev ? ev[1] : nullptr));
    if (res) {
        if (resident) *resident = P.nlaunch;
        return launch_resident(P, s, ev ? ev[2] : nullptr, ev ? ev[3] : nullptr);
    }
    return run_steps(L, r.a, pred_inter, pred, N, es, 1, T, s, ev);
}

}  // namespace

// A plan replays the captured section as one hipGraph, except on the resident path
// (step 1 + one resident launch per image group): there a graph launch costs more
// than the launches it saves (C2: 152.5 vs 147.3 us per step,
// tools/launch_probe.py), so the recorded launches are re-issued directly.
// NLSPN_PLAN_GRAPH=1 forces the graph.
struct nlspn_plan {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<LaunchRec> recs;
    bool direct = false;
    bool resident = false;  // holds a resident launch: res_guard applies around replays
};

extern "C" {

int nlspn_propagate_normalized(int dtype, const void *p0, const void *dep, const void *conf_eff,
                               const void *aff_norm, const void *off_ins, void *pred_inter, void *pred,
                               void *workspace, int B, int H, int W, int kh, int kw, int T, unsigned flags,
                               void *stream) {
    NLSPN_TRY(check_storage_dtype(dtype));
    NLSPN_TRY(check_nonempty(B, H, W));
    NLSPN_TRY(check_prop_time(T));
    if (!p0 || !aff_norm || !off_ins || !pred_inter || !pred) return fail(NLSPN_EINVAL, "null required pointer");
    const int K = kh * kw - 1;
    const long long HW = (long long)H * W, N = (long long)B * HW, off_bs = 2LL * (K + 1) * HW;
    const size_t es = esize(dtype);
    hipStream_t s = as_stream(stream);
    StepReq r{dtype, StepArgs{p0, conf_eff, dep, aff_norm, off_ins, pred_inter, T == 1 ? pred : nullptr,
                              (long long)(K + 1) * HW, off_bs, B, H, W, 0, 0, NLSPN_OFF_INSERTED, flags, nullptr, nullptr,
                              nullptr, nullptr, 0},
              kh, kw};
    StepLaunch L;
    NLSPN_TRY(prepare_step(r, L));
    ResPlan P;
    const ResInputs in{dtype, conf_eff, dep, aff_norm, off_ins, off_bs, pred_inter, pred, workspace, flags | kResOffInserted};
    const bool res = plan_resident(in, B, H, W, kh, kw, T, P);
    if (P.err) return P.err;
    StepArgs a1 = r.a;
    if (res) arm_resident(a1, P, pred_inter, N, es, T);
    NLSPN_TRY(launch(L, a1, s));
    if (res) return launch_resident(P, s);
    return run_steps(L, r.a, pred_inter, pred, N, es, 1, T, s, nullptr);
}

int nlspn_prop_step(int dtype, const void *p_in, const void *conf, const void *dep, const void *aff,
                    int64_t aff_bstride, const void *off, int64_t off_bstride, int off_layout, void *p_out,
                    void *pred_out, int B, int H, int W, int kh, int kw, unsigned flags, void *stream) {
    StepReq r{dtype, StepArgs{p_in, conf, dep, aff, off, p_out, pred_out, aff_bstride, off_bstride, B, H, W, 0, 0,
                              off_layout == NLSPN_OFF_RAW ? 1 : 0, flags, nullptr, nullptr, nullptr, nullptr, 0},
              kh, kw};
    StepLaunch L;
    NLSPN_TRY(prepare_step(r, L));
    return launch(L, r.a, as_stream(stream));
}

size_t nlspn_workspace_bytes(int dtype, int B, int H, int W) {
    (void)dtype; (void)B; (void)H; (void)W;
    return kSyncBytes;  // the resident kernel's sync words (the prologue needs no scratch)
}

int nlspn_propagate(int dtype, const void *pred_init, const void *dep, const void *conf, const void *aff_raw,
                    int64_t aff_bstride, const void *off_raw, int64_t off_bstride, const float *gamma,
                    void *pred_inter, void *pred, void *aff_out, void *off_out, void *conf_out, void *workspace,
                    int B, int H, int W, int kh, int kw, int T, int kind, unsigned flags, void *stream) {
    return propagate_impl(dtype, pred_init, dep, conf, aff_raw, aff_bstride, off_raw, off_bstride, gamma, pred_inter,
                          pred, aff_out, off_out, conf_out, workspace, B, H, W, kh, kw, T, kind, flags,
                          as_stream(stream), nullptr, nullptr);
}

int nlspn_plan_create(nlspn_plan_t *plan, int dtype, const void *pred_init, const void *dep, const void *conf,
                      const void *aff_raw, int64_t aff_bstride, const void *off_raw, int64_t off_bstride,
                      const float *gamma, void *pred_inter, void *pred, void *aff_out, void *off_out, void *conf_out,
                      void *workspace, int B, int H, int W, int kh, int kw, int T, int kind, unsigned flags) {
    if (!plan) return fail(NLSPN_EINVAL, "plan is null");
    *plan = nullptr;
    (void)dev_state();  // its one-time host allocation must not happen inside the capture
    // the resident kernel's sync words: zero before the plan's first launch (each launch leaves
    // them so); outside the capture
    if (workspace) NLSPN_HIP_TRY(hipMemset(workspace, 0, kSyncBytes));
    hipStream_t cs = nullptr;
    NLSPN_HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(cs);
        return fail(NLSPN_EHIP, "hipStreamBeginCapture: %s", hipGetErrorString(e));
    }
    std::vector<LaunchRec> recs;
    g_rec = &recs;
    int rc = nlspn_propagate(dtype, pred_init, dep, conf, aff_raw, aff_bstride, off_raw, off_bstride, gamma,
                             pred_inter, pred, aff_out, off_out, conf_out, workspace, B, H, W, kh, kw, T, kind,
                             flags, cs);
    g_rec = nullptr;
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(cs, &g);
    (void)hipStreamDestroy(cs);
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess) return fail(NLSPN_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    hipGraphExec_t ge = nullptr;
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        return fail(NLSPN_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    }
    nlspn_plan *p = new nlspn_plan;
    p->graph = g;
    p->exec = ge;
    for (const LaunchRec &r : recs) p->resident = p->resident || r.resident;
    p->direct = (p->resident || recs.size() <= 2) && !env_is("NLSPN_PLAN_GRAPH", '1');
    p->recs = std::move(recs);
    *plan = p;
    return NLSPN_OK;
}

int nlspn_plan_launch(nlspn_plan_t plan, void *stream) {
    if (!plan) return fail(NLSPN_EINVAL, "plan is null");
    hipStream_t s = as_stream(stream);
    if (!plan->direct) {
        if (plan->resident) NLSPN_TRY(res_guard_before(s));
        NLSPN_HIP_TRY(hipGraphLaunch(plan->exec, s));
        return plan->resident ? res_guard_after(s) : NLSPN_OK;
    }
    for (LaunchRec &r : plan->recs) {
        void *args[] = {r.resident ? static_cast<void *>(&r.ra) : static_cast<void *>(&r.sa)};
        if (r.resident) NLSPN_TRY(res_guard_before(s));
        NLSPN_HIP_TRY(hipLaunchKernel(r.fn, r.grid, r.block, args, r.lds, s));
        if (r.resident) NLSPN_TRY(res_guard_after(s));
    }
    return check_launch("nlspn_plan_launch");
}

int nlspn_plan_destroy(nlspn_plan_t plan) {
    if (!plan) return NLSPN_OK;
    if (plan->exec) (void)hipGraphExecDestroy(plan->exec);
    if (plan->graph) (void)hipGraphDestroy(plan->graph);
    delete plan;
    return NLSPN_OK;
}

int nlspn_time_prop_step(int dtype, const void *p_in, const void *conf, const void *dep, const void *aff,
                         int64_t aff_bstride, const void *off, int64_t off_bstride, int off_layout, void *p_out,
                         int B, int H, int W, int kh, int kw, unsigned flags, int reps, void *stream, float *mean_ms,
                         float *min_ms) {
    if (reps < 1 || !mean_ms || !min_ms) return fail(NLSPN_EINVAL, "reps must be >= 1 and outputs non-null");
    StepReq r{dtype, StepArgs{p_in, conf, dep, aff, off, p_out, nullptr, aff_bstride, off_bstride, B, H, W, 0, 0,
                              off_layout == NLSPN_OFF_RAW ? 1 : 0, flags, nullptr, nullptr, nullptr, nullptr, 0},
              kh, kw};
    StepLaunch L;
    NLSPN_TRY(prepare_step(r, L));
    hipStream_t s = as_stream(stream);
    TimingEvents te(2 * (size_t)reps);
    NLSPN_TRY(te.create());
    for (int i = 0; i < reps; ++i) NLSPN_TRY(launch(L, r.a, s, te.ev[2 * i], te.ev[2 * i + 1]));
    NLSPN_HIP_TRY(hipStreamSynchronize(s));
    double sum = 0.0;
    float mn = 1e30f;
    for (int i = 0; i < reps; ++i) {
        float ms = 0.f;
        NLSPN_TRY(te.elapsed(2 * (size_t)i, &ms));
        sum += ms;
        mn = ms < mn ? ms : mn;
    }
    *mean_ms = (float)(sum / reps);
    *min_ms = mn;
    return NLSPN_OK;
}

int nlspn_time_propagate(int dtype, const void *pred_init, const void *dep, const void *conf, const void *aff_raw,
                         int64_t aff_bstride, const void *off_raw, int64_t off_bstride, const float *gamma,
                         void *pred_inter, void *pred, void *aff_out, void *off_out, void *conf_out, void *workspace,
                         int B, int H, int W, int kh, int kw, int T, int kind, unsigned flags, int reps, void *stream,
                         float *first_ms, float *rest_ms, int *resident) {
    if (reps < 1 || T < 1 || !first_ms || !rest_ms) return fail(NLSPN_EINVAL, "reps/T must be >= 1, outputs non-null");
    hipStream_t s = as_stream(stream);
    TimingEvents te(2 * (size_t)T * reps);
    NLSPN_TRY(te.create());
    int res = 0;
    for (int i = 0; i < reps; ++i)
        NLSPN_TRY(propagate_impl(dtype, pred_init, dep, conf, aff_raw, aff_bstride, off_raw, off_bstride, gamma,
                                 pred_inter, pred, aff_out, off_out, conf_out, workspace, B, H, W, kh, kw, T, kind, flags,
                                 s, te.ev.data() + 2 * (size_t)T * i, &res));
    NLSPN_HIP_TRY(hipStreamSynchronize(s));
    double f = 0.0, r = 0.0;
    const int nrest = T < 2 ? 0 : (res ? 1 : T - 1);  // res: one interval over every resident launch
    for (int i = 0; i < reps; ++i) {
        for (int k = 0; k <= nrest; ++k) {
            float ms = 0.f;
            NLSPN_TRY(te.elapsed(2 * ((size_t)T * i + k), &ms));
            (k ? r : f) += ms;
        }
    }
    *first_ms = (float)(f / reps);
    *rest_ms = (float)(r / reps);
    if (resident) *resident = res;
    return NLSPN_OK;
}

int nlspn_resident_config(int dtype, int B, int H, int W, int kh, int kw, int T, int has_conf, int *grid,
                          int *block, int *lds_bytes) {
    ResPlan P;
    alignas(16) static char dummy[16];
    void *d = dummy;
    const ResInputs in{dtype, has_conf ? d : nullptr, d, d, d, 2LL * (kh * kw - 1) * H * W, d, d, d, NLSPN_PRESERVE_INPUT};
    if (!plan_resident(in, B, H, W, kh, kw, T, P)) return 0;
    if (grid) *grid = (int)P.rec.grid[0];
    if (block) *block = P.rec.S.nt;
    if (lds_bytes) *lds_bytes = (int)P.rec.lds;
    return 1;
}

int nlspn_resident_helper(int dtype, int B, int H, int W, int kh, int kw, int T, int has_conf, int has_off_out,
                          int *block) {
    // the plan of an nlspn_propagate call with aligned tensors and raw offsets
    if (block) *block = 0;
    ResPlan P;
    alignas(16) static char dummy[16];
    void *d = dummy;
    ResInputs in{dtype, has_conf ? d : nullptr, d, d, d, 2LL * (kh * kw - 1) * H * W, d, d, d, NLSPN_PRESERVE_INPUT,
                 has_off_out ? d : nullptr};
    in.has_first = true;
    in.pinit = d; in.conf_raw = has_conf ? d : nullptr; in.aff_raw = d; in.aff_bs = (long long)(kh * kw - 1) * H * W;
    alignas(16) static const float gamma = 1.f;
    in.gamma = &gamma; in.aff_out = d; in.conf_out = has_conf ? d : nullptr;
    if (!plan_resident(in, B, H, W, kh, kw, T, P)) return 0;
    const bool helper = (P.a[0].flags & kResHelper) != 0;
    if (block) *block = P.rec.S.nt + (helper ? 64 : 0);
    return helper ? 1 : 0;
}

int nlspn_resident_status(int clear) {
    DevState *d = dev_state();
    if (!d || !d->host_status) return 0;
    const unsigned v = __atomic_load_n(d->host_status, __ATOMIC_ACQUIRE);
    if (v && clear) __atomic_store_n(d->host_status, 0u, __ATOMIC_RELEASE);
    if (v)
        fail(NLSPN_EABORTED,
             "a resident propagation launch on this device aborted (a part waited past its spin limit: the grid "
             "was not co-resident); its outputs were filled with NaN");
    return v ? 1 : 0;
}

}  // extern "C"
