// C ABI (include/dau_conv.h) and pass orchestration.
//
// Sequencing follows what the reference does between its op boundary and its kernels
// (plugins/tensorflow/src/dau_conv_op.cpp:150-324, dau_conv_grad_op.cpp:115-318,
//  src/dau_conv/base_dau_conv_layer.cu:15-127 Forward_gpu, :130-363 Backward_gpu), minus
// the per-call handle creation, side streams, host syncs and workspace re-allocation.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "dau_common.hpp"
#include "dau_tiled.hpp"

using namespace dau;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define DAU_HIP(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(DAU_INTERNAL, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// bump allocator over the caller's workspace
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* p) : base(static_cast<char*>(p)) {}
    template <typename T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off = align_up(off + count * sizeof(T));
        return p;
    }
};

// image n0 of an activation tensor whose elements are esize bytes (float32, or bfloat16 / binary16 behind the float* of the ABI)
inline const float* slab_ptr(const float* base, size_t elements, size_t esize) {
    return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + elements * esize);
}
inline float* slab_ptr(float* base, size_t elements, size_t esize) {
    return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + elements * esize);
}

// unit_testing edge rule of the numpy oracle (dau_conv_test.py:110-136)
int edge_disabled(int size) {
    if (size >= 64) return size % 64 == 0;
    if (size >= 32) return size % 32 == 0;
    if (size >= 16) return size % 16 == 0;
    if (size >= 8) return size % 8 == 0;
    return 0;
}

}  // namespace

// The members of a set: the ways it can run a pass.  The exact tiled kernels exist in every bucket, the others in bucket 4 only.
// Within a pass kind the order is the order in which pick_candidates enqueues the members that go ahead of the bucket sets.
enum Member {
    kTiledGather,                // gather-sum (y and dx): the exact tiled kernels of the set's bucket
    kSplit2, kSplit3, kSplit4,   // ... the two-limb f16 dense GEMM of radius 2 / 3 / 4 (k_dense_split.hip: fp32 accuracy)
    kLine4, kLine8,              // ... its line forms, one row of 9 / 17 taps (DAU_FLAG_DENSE_SPLIT_LINE: calls whose units lie on a line)
    kBf16R3, kBf16R4,            // ... the densified bf16 implicit GEMM of radius 3 / 4 (k_dense_bf16.hip; DAU_FLAG_DENSE_BF16)
    kTiledDot,                   // parameter gradients: the exact tiled gather-dot
    kDotLine4, kDotLine8,        // ... the line forms of the next, horizontal radius 4 / 8 (DAU_FLAG_SPLIT_DOT_LINE: calls whose units lie on a line)
    kSplitDot,                   // ... the two-limb f16 GEMM with the bilinear corners as rows (k_split_dot.hip: fp32 accuracy)
    kWgradR3, kWgradR4,          // ... the bf16 dense correlations of radius 3 / 4 (k_dense_wgrad.hip; DAU_FLAG_DENSE_BF16)
    kNumMembers
};
enum PassKind { kGatherSum, kGatherDot };
// the entry points and the config type a member has: its function table below and its array in BucketSet
enum Family { kFamTiledGather, kFamDense, kFamTiledDot, kFamSplitDot, kFamWgrad };
// What a member is.  Every non-exact member has an arithmetic of its own and goes ahead of the bucket sets under its own guard,
// except the radius-4 bf16 members: they run in place of their set's exact kernels.
struct MemberInfo {
    int kind;        // PassKind
    int family;      // Family
    int slot;        // its row in the family's function table and config array
    int radius;      // the offsets a bucket-4 member covers (its device guard's upper end)
    bool ahead;      // goes ahead of the bucket sets
    bool line;       // a line form: runs the calls whose units lie on a line
    int info_bit;    // the bit of dau_conv_plan_info::gather_dense_split that reports it (-1: none)
};
constexpr MemberInfo kMember[kNumMembers] = {
    {kGatherSum, kFamTiledGather, 0, 0, false, false, -1},   // kTiledGather
    {kGatherSum, kFamDense, 0, 2, true, false, 2},           // kSplit2
    {kGatherSum, kFamDense, 1, 3, true, false, 3},           // kSplit3
    {kGatherSum, kFamDense, 2, 4, true, false, 4},           // kSplit4
    {kGatherSum, kFamDense, 3, 4, true, true, 6},            // kLine4
    {kGatherSum, kFamDense, 4, 8, true, true, 7},            // kLine8
    {kGatherSum, kFamDense, 5, 3, true, false, -1},          // kBf16R3
    {kGatherSum, kFamDense, 6, 4, false, false, -1},         // kBf16R4
    {kGatherDot, kFamTiledDot, 0, 0, false, false, -1},      // kTiledDot
    {kGatherDot, kFamSplitDot, 0, 4, true, true, 8},         // kDotLine4
    {kGatherDot, kFamSplitDot, 1, 8, true, true, 9},         // kDotLine8
    {kGatherDot, kFamSplitDot, 2, 4, true, false, -1},       // kSplitDot
    {kGatherDot, kFamWgrad, 0, 3, true, false, -1},          // kWgradR3
    {kGatherDot, kFamWgrad, 1, 4, false, false, -1},         // kWgradR4
};
constexpr int kRingInfoBit = 5;                              // likewise, the radius-3 + ring member (BucketSet::ring)
constexpr int kFirst[2] = {kTiledGather, kTiledDot}, kEnd[2] = {kTiledDot, kNumMembers};   // the members of a pass kind
// gather-sum directions, which are also their profile slots: y from x (S -> F) and dx from the error (F -> S)
enum Dir { kFwd, kDx };

// the dense gather-sum members kSplit2 .. kBf16R4, one set of entry points each
struct DenseFns {
    bool (*configure)(int, int, int, int, int, int, int, int, int, DenseConfig*);
    size_t (*workspace_bytes)(const DenseConfig&);
    void (*init)(const DenseConfig&);
    void (*prepare)(hipStream_t, const DenseConfig&, const float*, const float*, bool, const UnitRef*, void*, const Guard&);
    void (*run)(hipStream_t, const DenseConfig&, float*, void*, const Guard&, const Epilogue&);
};
// (the bf16-product forms take no epilogue: dau_conv_epilogue_supported refuses their plans)
template <void (*Run)(hipStream_t, const DenseConfig&, float*, void*, const Guard&)>
void run_plain(hipStream_t st, const DenseConfig& c, float* out, void* ws, const Guard& g, const Epilogue&) { Run(st, c, out, ws, g); }
const DenseFns kDense[] = {
    {s2::split_gather_configure, s2::split_gather_workspace_bytes, s2::split_gather_init, s2::split_gather_prepare, s2::split_gather_run},
    {s3::split_gather_configure, s3::split_gather_workspace_bytes, s3::split_gather_init, s3::split_gather_prepare, s3::split_gather_run},
    {s4::split_gather_configure, s4::split_gather_workspace_bytes, s4::split_gather_init, s4::split_gather_prepare, s4::split_gather_run},
    {l4::split_gather_configure, l4::split_gather_workspace_bytes, l4::split_gather_init, l4::split_gather_prepare, l4::split_gather_run},
    {l8::split_gather_configure, l8::split_gather_workspace_bytes, l8::split_gather_init, l8::split_gather_prepare, l8::split_gather_run},
    {r3::dense_gather_configure, r3::dense_gather_workspace_bytes, r3::dense_gather_init, r3::dense_gather_prepare, run_plain<r3::dense_gather_run>},
    {r4::dense_gather_configure, r4::dense_gather_workspace_bytes, r4::dense_gather_init, r4::dense_gather_prepare, run_plain<r4::dense_gather_run>},
};
constexpr int kNumDense = sizeof(kDense) / sizeof(kDense[0]);
// the two-limb gather-dot members kDotLine4, kDotLine8 and kSplitDot: the 2-D member has the entry points of its line forms
struct SplitDotFns {
    bool (*configure)(const Shape&, int, int, SplitDotConfig*);
    size_t (*workspace_bytes)(const SplitDotConfig&);
    void (*init)(const SplitDotConfig&);
    void (*prepare)(hipStream_t, const SplitDotConfig&, const float*, const float*, const float*, int, int, void*, const Guard&);
    void (*run)(hipStream_t, const SplitDotConfig&, const UnitRef*, float*, void*, const Guard&);
};
const SplitDotFns kSplitDotFns[] = {
    {d4::split_dot_configure, d4::split_dot_workspace_bytes, d4::split_dot_init, d4::split_dot_prepare, d4::split_dot_run},
    {d8::split_dot_configure, d8::split_dot_workspace_bytes, d8::split_dot_init, d8::split_dot_prepare, d8::split_dot_run},
    {split_dot_configure, split_dot_workspace_bytes, split_dot_init, split_dot_prepare, split_dot_run},
};
constexpr int kNumSplitDot = sizeof(kSplitDotFns) / sizeof(kSplitDotFns[0]);
// the bf16 dense parameter-gradient members kWgradR3, kWgradR4
struct WgradFns {
    bool (*configure)(const Shape&, int, bool, WgradConfig*);
    size_t (*workspace_bytes)(const WgradConfig&);
    void (*init)(const WgradConfig&);
    void (*run)(hipStream_t, const WgradConfig&, const float*, const float*, const float*, const UnitRef*, int, int, float*, void*,
                const Guard&, int);
};
const WgradFns kWgrad[] = {
    {r3::dense_wgrad_configure, r3::dense_wgrad_workspace_bytes, r3::dense_wgrad_init, r3::dense_wgrad_run},
    {r4::dense_wgrad_configure, r4::dense_wgrad_workspace_bytes, r4::dense_wgrad_init, r4::dense_wgrad_run},
};
static_assert(kMember[kBf16R4].slot == kNumDense - 1 && kMember[kSplitDot].slot == kNumSplitDot - 1 && kMember[kWgradR4].slot == 1,
              "a member's slot is its row in its family's function table");

// The kernels of one offset bucket.  A plan holds one set per bucket up to the static one (the bucket max_kernel_size allows);
// which set and member run is decided per call from the actual max|mu| (pick_candidates below).
struct BucketSet {
    int bucket = 0;
    bool has[kNumMembers] = {};   // the members this set holds
    TiledConfig tiled[2];         // [Dir]
    DenseConfig dense[kNumDense][2];   // [MemberInfo::slot][Dir]
    TiledDotConfig tiled_dot;
    SplitDotConfig sdot[kNumSplitDot]; // [MemberInfo::slot]
    WgradConfig wgrad[2];              // [MemberInfo::slot]
    // Batch slabs.  Every pass stages its whole input before it gathers; where that staged copy would exceed the workspace
    // budget (DAU_WORKSPACE_BUDGET_GB at plan creation, default 12: only the 512 x 512 configurations get there) the pass
    // runs slab by slab over the batch -- the configs above are made for `slab_*` images, the passes loop -- so that the
    // workspace holds one slab's staged copy.  Forward and dx are per-image; the parameter sums add up over the slabs.
    // Only the exact kernels and the dense gather-sum members run in slabs.
    int slab_gather = 0, slab_dot = 0;     // images per slab (the whole batch unless the budget says otherwise)
    // DAU_FLAG_DENSE_SPLIT_OUTLIERS (bucket 4, with kSplit3): calls within +-4 whose units beyond +-3 number at most ring_limit run
    // their gather-sum as the radius-3 GEMM plus the ring pass (k_dense_ring.hip) -- kSplit3's kernels under a guard of their own
    bool ring = false;
    unsigned ring_limit = 0;
    RingConfig ringcfg[2];        // [Dir]
    const DenseConfig& ring_dense(int dir) const { return dense[kMember[kSplit3].slot][dir]; }   // kSplit3's config, which the ring member runs on
};
// The outlier-unit count up to which the radius-3 + ring member runs, in thousandths of the plan's live units: the largest tested
// fraction at which its two gather-sum passes took at most 0.9 x what the members it stands in for take on the same inputs
// -- 1 %: 0.79 x at 0.1 %, 0.89 x at 1 %, 1.14 x at 3 % at the north-star layer (profiles/r9_ab_dense_outliers.jsonl).
constexpr int kRingLimitPermille = 10;
constexpr int kBuckets[] = {4, 8, 16, 18, 20, 24, 32};
constexpr int kNumBuckets = sizeof(kBuckets) / sizeof(kBuckets[0]);

// The one place that maps a member to its entry points and its config: f(workspace_bytes, init, config) for member m of a set
// (dir: a gather-sum member's direction).
template <class F>
auto with_member(const BucketSet& bs, int m, int dir, F&& f) {
    const int i = kMember[m].slot;
    switch (kMember[m].family) {
    case kFamTiledGather: return f(tiled_gather_workspace_bytes, tiled_gather_init, bs.tiled[dir]);
    case kFamDense: return f(kDense[i].workspace_bytes, kDense[i].init, bs.dense[i][dir]);
    case kFamTiledDot: return f(tiled_dot_workspace_bytes, tiled_dot_init, bs.tiled_dot);
    case kFamSplitDot: return f(kSplitDotFns[i].workspace_bytes, kSplitDotFns[i].init, bs.sdot[i]);
    default: return f(kWgrad[i].workspace_bytes, kWgrad[i].init, bs.wgrad[i]);
    }
}
// workspace the members of one pass kind need in a set: they run one after the other in the same memory
size_t pass_bytes(const BucketSet& bs, int kind, int dir = kFwd) {
    size_t need = 0;
    for (int m = kFirst[kind]; m < kEnd[kind]; ++m)
        if (bs.has[m]) need = std::max(need, with_member(bs, m, dir, [](auto bytes, auto, const auto& cfg) { return bytes(cfg); }));
    // the ring list and the fp32 partial sums of the slab, behind the radius-3 form's own workspace
    if (kind == kGatherSum && bs.ring) need = std::max(need, s3::split_gather_workspace_bytes(bs.ring_dense(dir)) + ring_workspace_bytes(bs.ringcfg[dir]));
    return need;
}

// Does the dense form of `taps` taps ((2r+1)^2; a line form: 2r+1) pay against the exact gather?  MFMA work per pass in fp32-rate
// MAC units: the dense GEMM runs its taps x 3 limb products at 16x the fp32 rate over the PADDED tile (8-row / 8-column blocks, 128 output channels, 16 input
// channels) plus its staging, at ~55 % of the f16 roof; the exact gather 4 MACs per live unit at ~60 % of the fp32 roof on maps
// of 32 pixels and more, ~45 % on smaller ones (measured, same box, gather + staging per pass against the exact gather: NS radius 3
// 5.4 + 0.5 against 8.9 ms at four units, radius 4 8.5 + 0.5 against 9.4; radius 2 2.9 + 0.5 against 5.4 at two units; C1 27 x 27
// radius 3 0.36 / 0.42 + 0.07 against 0.60 / 0.51).  On whole tiles radius 2 pays from two units per channel pair on, radius 3 from
// three, radius 4 from four.
bool split_pays(double taps, int Cin, int Cout, int G_live, int H, int W) {
    const double hp = (H + 7) / 8 * 8, wp = (W + 7) / 8 * 8, fp = (Cout + 127) / 128 * 128, sp = (Cin + 15) / 16 * 16;
    const double dense = hp * wp * (fp * sp * taps * 3.0 / 16.0 / 0.55 + sp * 430.0);
    const double exact = (double)H * W * Cout * Cin * G_live * 4.0 / ((H < 32 || W < 32) ? 0.45 : 0.60);
    return dense < 1.1 * exact;
}

struct dau_conv_plan {
    dau_conv_desc d;
    Shape sh;
    int bucket;        // static offset bucket R: the largest displacement max_kernel_size allows
    int blur_k;        // prefilter support
    int drop_col, drop_row;
    int algo_fwd, algo_bwd;
    int nsets = 0;             // bucket sets, ascending; sets[nsets - 1] is the static bucket
    BucketSet sets[kNumBuckets];
    bool dynamic = false;      // pick the set from the actual offsets (tiled kernels only)
    // pinned host mirror (HostStatus, dau_common.hpp): the status of the most recent completed call -- the offset-bucket hint
    // of the next call; a stale or torn value only costs speed, never correctness (the device-side guards decide which set
    // really runs) -- and the STICKY record of the worst status any completed call has left since the last report.
    HostStatus* host_status = nullptr;
    // dynamic-LDS limits raised on these devices (bit d: done on device d; the first call on a device does it behind the lock)
    mutable std::atomic<unsigned long long> attrs_devices{0};
    mutable std::mutex attrs_mutex;
    const BucketSet& top() const { return sets[nsets - 1]; }
    long units() const { return (long)sh.S * sh.G * sh.F; }
    // bytes per activation element: float32, or bfloat16 / binary16 behind the float* of the ABI
    size_t esize() const { return (d.flags & (DAU_FLAG_IO_BF16 | DAU_FLAG_IO_F16)) ? 2 : 4; }
    int act() const { return (d.flags & DAU_FLAG_IO_F16) ? kActF16 : (d.flags & DAU_FLAG_IO_BF16) ? kActBF16 : kActF32; }
    // optional benchmark timing (dau_conv_profile_begin/_end); mutable because the passes take a const plan
    mutable bool profiling = false;
    mutable std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events[DAU_PROFILE_SLOTS];
    mutable size_t prof_used[DAU_PROFILE_SLOTS] = {0, 0, 0};
    mutable int prof_passes[DAU_PROFILE_SLOTS] = {0, 0, 0};   // passes (a pass may take several window launches)
};

namespace {

// event bracket around one dominant kernel launch when profiling is on
struct ProfScope {
    const dau_conv_plan* p;
    int slot;
    hipStream_t st;
    hipEvent_t stop = nullptr;
    ProfScope(const dau_conv_plan* plan, int slot_, hipStream_t st_) : p(plan), slot(slot_), st(st_) {
        if (!p->profiling) return;
        auto& pool = p->prof_events[slot];
        size_t& used = p->prof_used[slot];
        if (used == pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            pool.emplace_back(a, b);
        }
        (void)hipEventRecord(pool[used].first, st);
        stop = pool[used].second;
        ++used;
    }
    ~ProfScope() {
        if (stop) (void)hipEventRecord(stop, st);
    }
};

// The candidates one call enqueues: a set, the member of it that runs, and the device guard under which it runs.  Without a
// hint (first call, dynamic selection off) it is the static set, unguarded.  With a hint -- max|mu| of the most recent completed
// call, read from pinned host memory without a sync -- it is the smallest set that covers the hint, guarded by (-1, R_hint],
// followed by the static set guarded by (R_hint, inf): the device decides between them from the max|mu| of THIS call, so
// results never depend on the hint.  This replaces the reference's blocking amax + D2H copy per call (dau_conv_op.cpp:223-253)
// and makes a layer with a large max_kernel_size but small offsets run the small-offset kernels (the reference's tests rely on
// that, dau_conv_test.py:433,436).
// That holds for the gather-sum passes (y, dx), whose sums run over the units of one output element in the table's order whatever
// the tile: every set gives the same bits.  The tiled gather-dot sums over the positions of a region, and the regions differ from
// set to set: its bits depend on the set.  The parameter-gradient pass therefore takes no hint: it enqueues EVERY set that holds the
// kernel, smallest first, each guarded by its own range of offsets, so that the set that runs -- the smallest that covers the
// call's max|mu| -- depends on the call alone, whatever other layers, streams or threads that share the plan left in the mirror
// (tests/test_gpu_concurrency.py).  It is the set a hint from the call's own previous offsets chose.
struct Candidate {
    const BucketSet* set;
    Guard guard;
    int member;   // Member
    bool ring = false;   // kSplit3 with the ring pass (BucketSet::ring)
};

// dau_conv_last_status has just reported the whole mirror: forget it, sticky record included.
void clear_host_status(const dau_conv_plan* p) {
    if (!p->host_status) return;
    volatile HostStatus* h = p->host_status;
    h->valid = 0u; h->nan_seen = 0u; h->max_abs_mu_bits = 0u; h->bad_max_abs_mu_bits = 0u; h->bad_nan_seen = 0u;
}
// dau_conv_check_status has just reported the status of ONE workspace's call: forget the "most recent call" part, and of the sticky
// record only what is this very report (the same out-of-range maximum, the NaN flag if this call had one) -- it may also hold the
// not-yet-reported error of another layer or stream that shares the plan, which dau_conv_last_status must still see.
void clear_reported_status(const dau_conv_plan* p, unsigned max_bits, bool nan_seen) {
    if (!p->host_status) return;
    volatile HostStatus* h = p->host_status;
    h->valid = 0u; h->nan_seen = 0u; h->max_abs_mu_bits = 0u;
    if (h->bad_max_abs_mu_bits == max_bits) h->bad_max_abs_mu_bits = 0u;
    if (nan_seen) h->bad_nan_seen = 0u;
}

// the error a reported status carries (DAU_OK: none)
int status_error(const dau_conv_plan* p, float mx, bool nan_seen) {
    if (nan_seen) return fail(DAU_FAILED_PRECONDITION, "DAUConvOp ERROR: got NaN value in offset (mu1,mu2) variable");
    if (mx > (float)p->bucket)
        return fail(DAU_INVALID_ARGUMENT,
                    "DAUConvOp ERROR: actual offsets (%.3f) larger than what max_kernel_size=%d allows (setup max_kernel_size "
                    "and dau_unit_border_bound correctly to avoid this)",
                    mx, p->d.max_kernel_size);
    return DAU_OK;
}

// The members whose ARITHMETIC differs (split, bf16-dense) go first, smallest radius first, on every call, hint or no hint, so that
// which arithmetic a call gets depends on its own offsets only.  A set that holds the radius-4 bf16 member runs it in place of
// its exact kernels: as the static set of a one-bucket plan, as the hinted set, or guarded by (lo, 4] ahead of them.
// With the radius-3 + ring member: it shares the offsets (3, 4] with what follows it -- the radius-4 member, the hinted or the static
// set -- and the call's outlier-unit count tells them apart: the ring member at most ring_limit, the others more (or offsets beyond 4).
// With line members (DAU_FLAG_DENSE_SPLIT_LINE): they go first, under (-1, 4] and (4, 8], and run where the call's table has no unit
// off the line; every member that follows and shares offsets with them runs there only where it has one -- the flag-off plan's kernels.
// The line members of the gather-dot (DAU_FLAG_SPLIT_DOT_LINE) likewise, on the count of the pass's own bare table (run_param_sums).
constexpr int kMaxCandidates = 14;   // (the most: 2 line + 2 ahead + the radius-4 dense member + 7 bucket sets, in a parameter-gradient pass)
int pick_candidates(const dau_conv_plan* p, const Status* dev_status, int kind, Candidate out[kMaxCandidates]) {
    const BucketSet* top = &p->top();
    const BucketSet* s0 = &p->sets[0];
    auto member_of = [&](const BucketSet* b) {               // the member that runs in place of the set's exact kernels, or those
        for (int m = kFirst[kind]; m < kEnd[kind]; ++m)
            if (kMember[m].radius && !kMember[m].ahead && b->has[m]) return m;
        return kFirst[kind];
    };
    out[0] = Candidate{top, Guard{nullptr, 0.0f, 0.0f}, member_of(top)};
    if (!p->dynamic) return 1;
    const BucketSet* hinted = nullptr;
    if (p->host_status && p->nsets >= 2) {
        const volatile HostStatus* h = p->host_status;
        float mx = -1.0f;
        if (h->valid == 1u && h->nan_seen == 0u) {
            const unsigned bits = h->max_abs_mu_bits;
            std::memcpy(&mx, &bits, sizeof(float));
        }
        if (mx >= 0.0f)
            for (int i = 0; i + 1 < p->nsets && !hinted; ++i)
                if (mx <= (float)p->sets[i].bucket && p->sets[i].has[kFirst[kind]]) hinted = &p->sets[i];
    }
    int n = 0;
    float lo = -1.0f;
    bool with_ring = false;
    int line_r = 0;                                          // the offsets the line members cover
    for (int m = kFirst[kind]; m < kEnd[kind]; ++m) {        // (smaller radius first)
        if (!(kMember[m].line && s0->has[m])) continue;
        Guard g{dev_status, (float)line_r - (line_r ? 0.0f : 1.0f), (float)kMember[m].radius};
        g.line = kMember[m].radius;
        out[n++] = Candidate{s0, g, m};
        line_r = kMember[m].radius;
    }
    auto add = [&](const BucketSet* b, int member, float hi) {
        Guard g{dev_status, lo, hi};
        if (lo < (float)line_r) g.line = -line_r;
        if (with_ring && lo < 4.0f) { g.cnt_lo = s0->ring_limit + 1; g.cnt_upto = 4.0f; }
        out[n++] = Candidate{b, g, member};
        lo = hi;
    };
    for (int m = kFirst[kind]; m < kEnd[kind]; ++m) {
        if (!(kMember[m].ahead && s0->has[m]) || kMember[m].line) continue;
        add(s0, m, (float)kMember[m].radius);
        if (m == kSplit3 && s0->ring) {
            Guard g{dev_status, 3.0f, 4.0f, 0u, s0->ring_limit};
            g.line = -line_r;
            out[n++] = Candidate{s0, g, kSplit3, true};
            with_ring = true;
        }
    }
    if (member_of(s0) != kFirst[kind] && hinted != s0 && s0 != top) add(s0, member_of(s0), (float)s0->bucket);
    if (kind == kGatherDot) {                                // by the call's own offsets alone (see Candidate)
        for (int i = 0; i + 1 < p->nsets; ++i)
            if (p->sets[i].has[kFirst[kind]] && lo < (float)p->sets[i].bucket)
                add(&p->sets[i], member_of(&p->sets[i]), (float)p->sets[i].bucket);
    } else if (hinted && lo < (float)hinted->bucket) add(hinted, member_of(hinted), (float)hinted->bucket);
    if (n == 0) return 1;                                    // no hint, nothing dense: the static set, unguarded
    add(top, member_of(top), INFINITY);
    return n;
}

// first call of a plan on a device: raise the dynamic-LDS limit of every kernel its sets can launch (function attributes are
// per device, hence not at plan creation, which must also work without a device).  Plans are shared between threads (the
// TF plan cache hands one plan to every Compute of a shape): the first call on a device does this behind the plan's lock.
int ensure_attrs(const dau_conv_plan* p) {
    int dev = 0;
    DAU_HIP(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (p->attrs_devices.load(std::memory_order_acquire) & bit) return DAU_OK;
    std::lock_guard<std::mutex> lock(p->attrs_mutex);
    if (p->attrs_devices.load(std::memory_order_relaxed) & bit) return DAU_OK;
    (void)hipGetLastError();
    for (int i = 0; i < p->nsets; ++i) {
        const BucketSet& bs = p->sets[i];
        for (int m = 0; m < kNumMembers; ++m) {
            if (!bs.has[m]) continue;
            for (int dir = kFwd; dir <= (kMember[m].kind == kGatherSum ? kDx : kFwd); ++dir)   // (a gather-sum member: both directions)
                with_member(bs, m, dir, [](auto, auto init, const auto& cfg) { init(cfg); });
        }
        if (bs.ring) ring_init();
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return fail(DAU_INTERNAL, "raising the dynamic-LDS limit of the bucket-%d kernels failed: %s", bs.bucket,
                        hipGetErrorString(e));
    }
    p->attrs_devices.fetch_or(bit, std::memory_order_release);
    return DAU_OK;
}

// workspace of a tiled pass: the largest need of any set (the candidates run one after the other in the same memory)
size_t tiled_pass_bytes(const dau_conv_plan* p, int kind, int dir = kFwd) {
    size_t need = 0;
    for (int i = 0; i < p->nsets; ++i) need = std::max(need, pass_bytes(p->sets[i], kind, dir));
    return need;
}

struct FwdWs {
    Status* status;
    float* filters;
    UnitRef* table;
    void* gather;       // tiled: staged planes + packed units; direct: blurred input, NCHW
    size_t bytes;
};

FwdWs carve_forward(const dau_conv_plan* p, void* ws) {
    Carver c(ws);
    FwdWs w{};
    w.status = c.take<Status>(1);
    w.filters = c.take<float>(kFilterFloats);
    w.table = c.take<UnitRef>(p->units());
    if (p->algo_fwd == DAU_ALGO_TILED) w.gather = c.take<char>(tiled_pass_bytes(p, kGatherSum, kFwd));
    else w.gather = c.take<float>((size_t)p->sh.N * p->sh.S * p->sh.H * p->sh.W);
    w.bytes = c.off;
    return w;
}

struct BwdWs {
    Status* status;
    float* filters;
    UnitRef* table_bare;   // [S][G][F], w = 1  (parameter gradients)
    UnitRef* table_t;      // [F][G][S], negated offsets, times w  (input gradient)
    float* r4;             // [4][S][G][F]
    float* xk4;            // direct: [N*S][4][H][W]
    void* gather_dx;       // tiled: staged planes + packed units; direct: blurred error, NCHW
    void* tiled_dot;
    size_t bytes;
};

BwdWs carve_backward(const dau_conv_plan* p, void* ws) {
    Carver c(ws);
    BwdWs w{};
    const Shape& s = p->sh;
    w.status = c.take<Status>(1);
    w.filters = c.take<float>(kFilterFloats);
    w.table_bare = c.take<UnitRef>(p->units());
    w.table_t = c.take<UnitRef>(p->units());
    w.r4 = c.take<float>(kNumK * p->units());
    if (p->algo_bwd == DAU_ALGO_TILED) w.tiled_dot = c.take<char>(tiled_pass_bytes(p, kGatherDot));
    else w.xk4 = c.take<float>((size_t)kNumK * s.N * s.S * s.H * s.W);
    if (p->algo_fwd == DAU_ALGO_TILED) w.gather_dx = c.take<char>(tiled_pass_bytes(p, kGatherSum, kDx));
    else w.gather_dx = c.take<float>((size_t)s.N * s.F * s.H * s.W);
    w.bytes = c.off;
    return w;
}

// One gather-sum pass: y from x (kFwd: S -> F, unit table [S][G][F]) or dx from the error (kDx: F -> S, mirrored Gaussian, table
// [F][G][S] with negated offsets).  `ws`: the tiled workspace, or the direct path's blurred copy.
// epi (tiled plans, kFwd): the fused epilogue of the stores; a pass of several offset windows gives it to the last window's store.
// Its residual is indexed like `out`: a batch slab reads the images it writes.  Likewise its gate (kDx of a DAU_FLAG_INPUT_RELU plan: the raw x).
void run_gather_sum(const dau_conv_plan* p, hipStream_t st, int dir, const float* in, float* out, const float* filters,
                    const UnitRef* table, Status* status, void* ws, const Epilogue& epi = Epilogue{}) {
    const Shape& s = p->sh;
    const int cin = dir == kFwd ? s.S : s.F, cout = dir == kFwd ? s.F : s.S;
    const bool mirrored = dir == kDx;
    if (p->profiling) ++p->prof_passes[dir];
    if (p->algo_fwd != DAU_ALGO_TILED) {
        launch_blur_direct(st, in, (long)s.N * cin, s.H, s.W, filters + (mirrored ? 5 : 0) * kFilterPlane, 1, p->blur_k,
                           static_cast<float*>(ws));
        ProfScope prof(p, dir, st);
        launch_gather_sum_direct(st, static_cast<float*>(ws), table, s.N, cin, cout, s.G, s.H, s.W, out);
        return;
    }
    Candidate cand[kMaxCandidates];
    const int ncand = pick_candidates(p, status, kGatherSum, cand);
    for (int ci = 0; ci < ncand; ++ci) {
        const BucketSet& bs = *cand[ci].set;
        const Guard& g = cand[ci].guard;
        const int m = cand[ci].member;
        const bool ring = cand[ci].ring;
        // the ring member's list and partial sums lie behind the radius-3 form's workspace; the list is built once per pass
        void* ring_ws = ring ? static_cast<char*>(ws) + s3::split_gather_workspace_bytes(bs.ring_dense(dir)) : nullptr;
        if (ring) ring_build_list(st, bs.ringcfg[dir], table, ring_ws, g);
        for (int n0 = 0; n0 < s.N; n0 += bs.slab_gather) {                 // one slab unless the staged copy exceeds the budget
            const float* ins = slab_ptr(in, (size_t)n0 * cin * s.H * s.W, p->esize());
            float* outs = slab_ptr(out, (size_t)n0 * cout * s.H * s.W, p->esize());
            Epilogue epis = epi;
            if (epi.residual) epis.residual = slab_ptr(epi.residual, (size_t)n0 * cout * s.H * s.W, p->esize());
            if (epi.gate) epis.gate = slab_ptr(epi.gate, (size_t)n0 * cout * s.H * s.W, p->esize());
            if (m == kTiledGather) {
                const TiledConfig& cfg = bs.tiled[dir];
                const int nwin = tiled_gather_windows(cfg);
                for (int window = 0; window < nwin; ++window) {   // one pass unless the bucket is 32
                    tiled_gather_prepare(st, cfg, ins, filters, mirrored, table, ws, window, g);
                    ProfScope prof(p, dir, st);
                    tiled_gather_run(st, cfg, outs, ws, window > 0, g, window + 1 == nwin ? epis : Epilogue{});
                }
            } else {                                                       // a dense member: one GEMM per slab
                const DenseFns& fn = kDense[kMember[m].slot];
                const DenseConfig& cfg = bs.dense[kMember[m].slot][dir];
                fn.prepare(st, cfg, ins, filters, mirrored, table, ws, g);
                ProfScope prof(p, dir, st);
                if (ring) {                                                // the ring pass, then the GEMM whose epilogue adds its sums
                    ring_run(st, bs.ringcfg[dir], s3::split_gather_staged(cfg, ws), ring_ws, status, g);
                    s3::split_gather_run_add(st, cfg, outs, ring_partial(bs.ringcfg[dir], ring_ws), ws, g, epis);
                } else {
                    fn.run(st, cfg, outs, ws, g, epis);
                }
            }
        }
    }
}

// The flag rules of a desc, in the order in which they are checked: a desc that sets any of `flags` must set all of `needs` and
// none of `excludes`.
struct FlagRule {
    int flags, needs, excludes;
    const char* message;
};
constexpr int kWgradFlags = DAU_FLAG_DENSE_WGRAD_NEVER | DAU_FLAG_DENSE_WGRAD_ALWAYS;
constexpr int kNoSplitFlags = DAU_FLAG_DENSE_BF16 | DAU_FLAG_NO_DENSE_SPLIT;
constexpr FlagRule kFlagRules[] = {
    {DAU_FLAG_IO_F16, 0, DAU_FLAG_IO_BF16 | DAU_FLAG_DENSE_BF16 | kWgradFlags,
     "DAU_FLAG_IO_F16 excludes DAU_FLAG_IO_BF16, DAU_FLAG_DENSE_BF16 and DAU_FLAG_DENSE_WGRAD_NEVER / _ALWAYS"},
    {DAU_FLAG_DENSE_BF16, DAU_FLAG_IO_BF16, 0, "DAU_FLAG_DENSE_BF16 needs DAU_FLAG_IO_BF16 (it is the bf16 layer's gather-sum)"},
    {DAU_FLAG_DENSE_SPLIT_F16, 0, kNoSplitFlags, "DAU_FLAG_DENSE_SPLIT_F16 excludes DAU_FLAG_DENSE_BF16 and DAU_FLAG_NO_DENSE_SPLIT"},
    {DAU_FLAG_DENSE_SPLIT_OUTLIERS, 0, kNoSplitFlags, "DAU_FLAG_DENSE_SPLIT_OUTLIERS excludes DAU_FLAG_DENSE_BF16 and DAU_FLAG_NO_DENSE_SPLIT"},
    {DAU_FLAG_DENSE_SPLIT_LINE, DAU_FLAG_SINGLE_DIM_KERNEL, 0, "DAU_FLAG_DENSE_SPLIT_LINE needs DAU_FLAG_SINGLE_DIM_KERNEL"},
    {DAU_FLAG_DENSE_SPLIT_LINE, 0, kNoSplitFlags, "DAU_FLAG_DENSE_SPLIT_LINE excludes DAU_FLAG_DENSE_BF16 and DAU_FLAG_NO_DENSE_SPLIT"},
    {DAU_FLAG_SPLIT_DOT_LINE, DAU_FLAG_SINGLE_DIM_KERNEL, 0, "DAU_FLAG_SPLIT_DOT_LINE needs DAU_FLAG_SINGLE_DIM_KERNEL"},
    {DAU_FLAG_SPLIT_DOT_LINE, DAU_FLAG_USE_INTERPOLATION, 0, "DAU_FLAG_SPLIT_DOT_LINE needs DAU_FLAG_USE_INTERPOLATION"},
    {DAU_FLAG_SPLIT_DOT_LINE, 0, kNoSplitFlags, "DAU_FLAG_SPLIT_DOT_LINE excludes DAU_FLAG_DENSE_BF16 and DAU_FLAG_NO_DENSE_SPLIT"},
    {kWgradFlags, DAU_FLAG_DENSE_BF16, 0, "DAU_FLAG_DENSE_WGRAD_NEVER / _ALWAYS qualify DAU_FLAG_DENSE_BF16 and exclude each other"},
    {DAU_FLAG_DENSE_WGRAD_NEVER, 0, DAU_FLAG_DENSE_WGRAD_ALWAYS, "DAU_FLAG_DENSE_WGRAD_NEVER / _ALWAYS qualify DAU_FLAG_DENSE_BF16 and exclude each other"},
    {DAU_FLAG_IO_NHWC, 0, DAU_FLAG_DENSE_BF16 | kWgradFlags, "DAU_FLAG_IO_NHWC excludes DAU_FLAG_DENSE_BF16 and DAU_FLAG_DENSE_WGRAD_NEVER / _ALWAYS"},
    {DAU_FLAG_INPUT_RELU, 0, DAU_FLAG_DENSE_BF16, "DAU_FLAG_INPUT_RELU excludes DAU_FLAG_DENSE_BF16 (the bf16-product forms have no input prologue)"},
};

// (a) what a desc must satisfy whatever the kernels support; gives the static offset bucket and the prefilter support
int validate_desc(const dau_conv_desc* desc, int& bucket, int& blur_k) {
    if (desc->struct_size != (int32_t)sizeof(dau_conv_desc))
        return fail(DAU_INVALID_ARGUMENT, "dau_conv_desc.struct_size %d != %zu", desc->struct_size, sizeof(dau_conv_desc));
    if (desc->batch < 1 || desc->in_channels < 1 || desc->out_channels < 1 || desc->units_per_channel < 1 ||
        desc->height < 1 || desc->width < 1)
        return fail(DAU_INVALID_ARGUMENT, "all of N,S,F,G,H,W must be >= 1");
    if (desc->number_units_ignore < 0 || desc->number_units_ignore >= desc->units_per_channel)
        return fail(DAU_INVALID_ARGUMENT, "number_units_ignore must be in [0, G)");
    if (desc->max_kernel_size < 3 || desc->max_kernel_size % 2 == 0)
        return fail(DAU_INVALID_ARGUMENT, "kernel_size must be odd and >= 3");
    // offset bucket from the largest displacement the attrs allow (dau_conv_op.cpp:236-253)
    bucket = 0;
    for (int b : kBuckets)
        if (!bucket && desc->max_kernel_size / 2 <= b) bucket = b;
    if (!bucket)
        return fail(DAU_INVALID_ARGUMENT,
                    "DAUConv: offsets larger than the 32 px the kernels stage (set max_kernel_size <= 65)");
    if (!(desc->sigma_hint > 0.0f))  // DAU_CHECK(sigma > 0) base_dau_conv_layer.cpp:143
        return fail(DAU_FAILED_PRECONDITION, "Must use sigma > 0 - initialize it with appropriate value");
    blur_k = dau_conv_filter_support(desc->sigma_hint);
    if (blur_k > kMaxBlurSupport)
        return fail(DAU_INVALID_ARGUMENT, "sigma %.3f needs a %dx%d prefilter; at most %dx%d is supported", desc->sigma_hint,
                    blur_k, blur_k, kMaxBlurSupport, kMaxBlurSupport);
    if (desc->algo < DAU_ALGO_AUTO || desc->algo > DAU_ALGO_TILED) return fail(DAU_INVALID_ARGUMENT, "unknown algo");
    for (const FlagRule& r : kFlagRules)
        if ((desc->flags & r.flags) && ((desc->flags & r.needs) != r.needs || (desc->flags & r.excludes)))
            return fail(DAU_INVALID_ARGUMENT, "%s", r.message);
    return DAU_OK;
}

// (b) the members and configs of the set of bs.bucket
void configure_set(const dau_conv_plan& p, double budget_bytes, BucketSet& bs) {
    const Shape& s = p.sh;
    const int flags = p.d.flags, b = bs.bucket, blur_k = p.blur_k, act = p.act(), ignore = p.d.number_units_ignore;
    const bool want_dense = (flags & DAU_FLAG_DENSE_BF16) && p.d.algo != DAU_ALGO_DIRECT;
    const bool split_forced = (flags & DAU_FLAG_DENSE_SPLIT_F16) != 0;
    const bool split_allowed = !(flags & kNoSplitFlags) && p.d.algo != DAU_ALGO_DIRECT;
    const int g_live = s.G - ignore;
    const long live_units = (long)s.S * s.F * g_live, ignored_units = (long)s.S * s.F * ignore;
    // a line member of radius 8 is held where the plan's offsets reach it and the one of radius 4 (the member before it) is held
    // (DAU_FLAG_STATIC_BUCKET: no per-call selection, the line flags are inert as the outliers flag is)
    auto line_wanted = [&](int m, int flag) {
        return (flags & flag) && !(flags & DAU_FLAG_STATIC_BUCKET) && (kMember[m].radius == 4 || (p.bucket >= 8 && bs.has[m - 1]));
    };
    // does the dense gather-sum form of `taps` taps pay in both directions (or is it forced)
    auto pays = [&](double taps) {
        return split_forced || (split_pays(taps, s.S, s.F, g_live, s.H, s.W) && split_pays(taps, s.F, s.S, g_live, s.H, s.W));
    };
    // both directions of dense gather-sum member m, for n images
    auto configure_dense = [&](int m, int n) {
        const int i = kMember[m].slot, r = kMember[m].radius;
        return kDense[i].configure(n, s.S, s.F, s.G, s.H, s.W, r, blur_k, act, &bs.dense[i][kFwd]) &&
               kDense[i].configure(n, s.F, s.S, s.G, s.H, s.W, r, blur_k, act, &bs.dense[i][kDx]);
    };
    auto configure_gather = [&](int n) {
        bs.has[kTiledGather] = tiled_gather_configure(n, s.S, s.F, s.G, s.H, s.W, b, blur_k, act, &bs.tiled[kFwd]) &&
                               tiled_gather_configure(n, s.F, s.S, s.G, s.H, s.W, b, blur_k, act, &bs.tiled[kDx]);
        const bool dense_set = b == 4 && bs.has[kTiledGather];   // the dense members: bucket 4 only
        // downwards, as the bf16 radius-3 member needs the radius-4 one
        for (int m = kBf16R4; m >= kSplit2; --m) {
            if (kMember[m].line) continue;                   // (below)
            const double side = 2.0 * kMember[m].radius + 1;
            const bool want = m == kBf16R4 ? want_dense : m == kBf16R3 ? bs.has[kBf16R4] : split_allowed && pays(side * side);
            bs.has[m] = dense_set && want && configure_dense(m, n);
        }
        // the line members: bucket 4's set like the others
        for (int m = kLine4; m <= kLine8; ++m)
            bs.has[m] = dense_set && line_wanted(m, DAU_FLAG_DENSE_SPLIT_LINE) && split_allowed && pays(2.0 * kMember[m].radius + 1) &&
                        configure_dense(m, n);
        // radius 3 + ring: where the radius-3 member is; its list holds the entries of ring_limit live units and of the ignored ones
        // (the input-gradient table ignores no unit, and the count leaves them out)
        bs.ring = (flags & DAU_FLAG_DENSE_SPLIT_OUTLIERS) && bs.has[kSplit3];
        if (bs.ring) {
            bs.ring_limit = (unsigned)(live_units * DAU_TUNE_INT("DAU_RING_LIMIT_PERMILLE", kRingLimitPermille) / 1000);
            for (int dir : {kFwd, kDx}) ring_configure(bs.ring_dense(dir), (long)bs.ring_limit + ignored_units, &bs.ringcfg[dir]);
        }
        return std::max(pass_bytes(bs, kGatherSum, kFwd), pass_bytes(bs, kGatherSum, kDx));
    };
    auto configure_dot = [&](int n) {
        Shape sn = s; sn.N = n;
        bs.has[kTiledDot] = tiled_dot_configure(sn, b, blur_k, act, ignore, &bs.tiled_dot);
        return pass_bytes(bs, kGatherDot);
    };
    // (c) slab candidates: the whole batch, then its even divisors (image pairs stay together), largest first
    auto pick_slab = [&](auto&& configure) {
        int chosen = s.N;
        for (int n = s.N; n >= 2; --n) {
            if (s.N % n || (n != s.N && (n & 1))) continue;
            chosen = n;
            if ((double)configure(n) <= budget_bytes) break;
        }
        configure(chosen);
        return chosen;
    };
    bs.slab_gather = pick_slab(configure_gather);
    bs.slab_dot = pick_slab(configure_dot);
    const bool whole_dot = b == 4 && bs.has[kTiledDot] && bs.slab_dot == s.N;
    // dense parameter gradients: the bf16-dense layer's bucket-4 set, whole batch in one slab, three or more units (its cost
    // does not depend on the unit count: 15.3 ms at the north-star size against 16.0 ms for the exact gather-dot of a
    // four-unit block, 9.7 ms of two units); DAU_FLAG_DENSE_WGRAD_NEVER / _ALWAYS: never / from one unit on.  The radius-3
    // form where the radius-4 one and the radius-3 gather-sum are there.
    const int min_units = (flags & DAU_FLAG_DENSE_WGRAD_NEVER) ? 1 << 30 : (flags & DAU_FLAG_DENSE_WGRAD_ALWAYS) ? 1 : 3;
    for (int m = kWgradR4; m >= kWgradR3; --m) {
        const WgradFns& fn = kWgrad[kMember[m].slot];
        WgradConfig& cfg = bs.wgrad[kMember[m].slot];
        const bool want = m == kWgradR4 ? whole_dot && bs.has[kBf16R4] && s.G >= min_units : bs.has[kWgradR4] && bs.has[kBf16R3];
        bs.has[m] = want && fn.configure(s, blur_k, (flags & DAU_FLAG_IO_BF16) != 0, &cfg) && (double)fn.workspace_bytes(cfg) <= budget_bytes;
    }
    // two-limb f16 gather-dot: bucket 4, interpolation on, the whole batch in one pass; by default where the blocks of four
    // units per channel pair are at least 3/4 full (G = 3, 4, 7, 8, ...), with DAU_FLAG_DENSE_SPLIT_F16 whatever the unit
    // count.  fp32, f16 and bf16 layers alike; a bf16 layer's error is staged in one limb (split_dot_configure).  The 2-D
    // member for 2-D units; its line members (DAU_FLAG_SPLIT_DOT_LINE, single-dimension layers) are held where it would be.
    const bool interp2d = (flags & DAU_FLAG_USE_INTERPOLATION) && !(flags & DAU_FLAG_SINGLE_DIM_KERNEL);
    const bool fill = 4 * s.G >= 3 * 4 * ((s.G + 3) / 4);
    for (int m = kDotLine4; m <= kSplitDot; ++m) {
        const SplitDotFns& fn = kSplitDotFns[kMember[m].slot];
        SplitDotConfig& cfg = bs.sdot[kMember[m].slot];
        const bool want = kMember[m].line ? line_wanted(m, DAU_FLAG_SPLIT_DOT_LINE) : interp2d;
        bs.has[m] = split_allowed && whole_dot && (split_forced || fill) && want && fn.configure(s, blur_k, act, &cfg) &&
                    (double)fn.workspace_bytes(cfg) <= budget_bytes;
    }
    // Storage format of the activations: an f16 plan configures every member exactly as the fp32 plan of the same desc does (the
    // staged copies are fp32 in both), only the loads of x / dy and the stores of y / dx differ.  Likewise the layout: an NHWC
    // plan is the NCHW plan of the same desc, its configs marked here, after they are made (addresses only).  And the input ReLU:
    // the plan of the same desc, the configs that stage x (forward gather-sum, parameter gradients) marked.  (The bf16-product
    // forms read neither mark: plan creation refuses them together with these flags.)
    const int nhwc = (flags & DAU_FLAG_IO_NHWC) != 0, in_relu = (flags & DAU_FLAG_INPUT_RELU) != 0;
    auto mark = [&](auto& cfg, bool stages_x) { cfg.nhwc = nhwc; cfg.in_relu = stages_x && in_relu; };
    for (int dir : {kFwd, kDx}) {
        mark(bs.tiled[dir], dir == kFwd);
        for (DenseConfig* cfg : bs.dense) mark(cfg[dir], dir == kFwd);
    }
    mark(bs.tiled_dot, true);
    for (SplitDotConfig& cfg : bs.sdot) mark(cfg, true);
}

// (d) what the plan's flags and algo need of the sets that were made; then the algorithms and the per-call selection
int finish_plan(dau_conv_plan* p) {
    const int flags = p->d.flags, algo = p->d.algo;
    const bool fwd_ok = p->top().has[kTiledGather], dot_ok = p->top().has[kTiledDot];
    const struct { int flag; const char* name; } tiled_only[] = {
        {DAU_FLAG_IO_F16, "DAU_FLAG_IO_F16"}, {DAU_FLAG_IO_BF16, "DAU_FLAG_IO_BF16"}, {DAU_FLAG_IO_NHWC, "DAU_FLAG_IO_NHWC"},
        {DAU_FLAG_INPUT_RELU, "DAU_FLAG_INPUT_RELU"}};
    for (const auto& t : tiled_only)
        if ((flags & t.flag) && (algo == DAU_ALGO_DIRECT || !(fwd_ok && dot_ok)))
            return fail(DAU_INVALID_ARGUMENT, "%s needs the tiled kernels, which do not support this shape / algo", t.name);
    if (algo == DAU_ALGO_TILED && !(fwd_ok && dot_ok)) return fail(DAU_INVALID_ARGUMENT, "DAU_ALGO_TILED does not support this shape");
    p->algo_fwd = (algo != DAU_ALGO_DIRECT && fwd_ok) ? DAU_ALGO_TILED : DAU_ALGO_DIRECT;
    p->algo_bwd = (algo != DAU_ALGO_DIRECT && dot_ok) ? DAU_ALGO_TILED : DAU_ALGO_DIRECT;
    // dynamic selection: tiled kernels, more than one bucket or a member that goes ahead of the sets, not switched off
    // (DAU_FLAG_STATIC_BUCKET)
    bool ahead = false;
    for (int m = 0; m < kNumMembers; ++m) ahead = ahead || (kMember[m].ahead && p->sets[0].has[m]);
    p->dynamic = (p->nsets > 1 || ahead) && !(flags & DAU_FLAG_STATIC_BUCKET) &&
                 (p->algo_fwd == DAU_ALGO_TILED || p->algo_bwd == DAU_ALGO_TILED);
    if (!p->dynamic || p->algo_fwd != DAU_ALGO_TILED) p->sets[0].ring = false;   // no per-call selection: the flag is inert
    return DAU_OK;
}

}  // namespace

extern "C" {

int dau_conv_abi_version(void) { return DAU_CONV_ABI_VERSION; }

#ifndef DAU_BUILD_ID
#define DAU_BUILD_ID "unknown"
#endif
const char* dau_conv_build_id(void) { return DAU_BUILD_ID; }

const char* dau_conv_last_error(void) { return g_last_error.c_str(); }

int dau_conv_filter_support(float sigma) { return 2 * (int)std::ceil(5.0f * sigma) + 1; }   // base_dau_conv_layer.cpp:146

int dau_conv_plan_create(const dau_conv_desc* desc, dau_conv_plan** plan_out) {
    if (!desc || !plan_out) return fail(DAU_INVALID_ARGUMENT, "null argument");
    int bucket, blur_k;
    if (int rc = validate_desc(desc, bucket, blur_k)) return rc;

    std::unique_ptr<dau_conv_plan> p(new (std::nothrow) dau_conv_plan());
    if (!p) return fail(DAU_INTERNAL, "out of host memory");
    p->d = *desc;
    p->sh = Shape{desc->batch, desc->in_channels, desc->out_channels, desc->units_per_channel, desc->height, desc->width};
    p->bucket = bucket;
    p->blur_k = blur_k;
    const bool ut = desc->flags & DAU_FLAG_UNIT_TESTING;
    p->drop_col = ut ? edge_disabled(desc->width) : 0;
    p->drop_row = ut ? edge_disabled(desc->height) : 0;

    const char* budget_env = getenv("DAU_WORKSPACE_BUDGET_GB");
    const double budget_bytes = (budget_env ? atof(budget_env) : 12.0) * 1e9;
    for (int b : kBuckets) {
        if (b > bucket) break;
        BucketSet& bs = p->sets[p->nsets++];
        bs.bucket = b;
        configure_set(*p, budget_bytes, bs);
    }
    if (int rc = finish_plan(p.get())) return rc;
    // The pinned status mirror needs a device; without one (header-only checks on a CPU box) the plan simply has no hint.
    void* hs = nullptr;
    // portable + mapped: a plan may be used on any device, and every device's prepare_units_kernel writes the mirror
    if (hipHostMalloc(&hs, sizeof(HostStatus), hipHostMallocPortable | hipHostMallocMapped) == hipSuccess && hs) {
        std::memset(hs, 0, sizeof(HostStatus));
        p->host_status = static_cast<HostStatus*>(hs);
    } else {
        (void)hipGetLastError();   // no device: not an error of this call
    }
    *plan_out = p.release();
    return DAU_OK;
}

int dau_conv_plan_destroy(dau_conv_plan* plan) {
    if (plan) {
        for (auto& pool : plan->prof_events)
            for (auto& ev : pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        if (plan->host_status) (void)hipHostFree(plan->host_status);
    }
    delete plan;
    return DAU_OK;
}

int dau_conv_profile_begin(dau_conv_plan* plan) {
    if (!plan) return fail(DAU_INVALID_ARGUMENT, "null argument");
    for (size_t& u : plan->prof_used) u = 0;
    for (int& n : plan->prof_passes) n = 0;
    plan->profiling = true;
    return DAU_OK;
}

int dau_conv_profile_end(dau_conv_plan* plan, double* ms_out, int32_t* passes_out) {
    if (!plan || !ms_out || !passes_out) return fail(DAU_INVALID_ARGUMENT, "null argument");
    plan->profiling = false;
    for (int slot = 0; slot < DAU_PROFILE_SLOTS; ++slot) {
        double total = 0.0;
        for (size_t i = 0; i < plan->prof_used[slot]; ++i) {
            auto& ev = plan->prof_events[slot][i];
            DAU_HIP(hipEventSynchronize(ev.second));
            float ms = 0.0f;
            DAU_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
            total += ms;
        }
        ms_out[slot] = total;
        passes_out[slot] = plan->prof_passes[slot];
        plan->prof_used[slot] = 0;
        plan->prof_passes[slot] = 0;
    }
    return DAU_OK;
}

int dau_conv_plan_get_info(const dau_conv_plan* plan, dau_conv_plan_info* info) {
    if (!plan || !info) return fail(DAU_INVALID_ARGUMENT, "null argument");
    info->offset_bucket = plan->bucket;
    info->blur_support = plan->blur_k;
    info->algo_forward = plan->algo_fwd;
    info->algo_backward = plan->algo_bwd;
    info->drop_last_col = plan->drop_col;
    info->drop_last_row = plan->drop_row;
    const BucketSet& top = plan->top();
    const bool* s0 = plan->sets[0].has;
    const bool tiled_fwd = plan->algo_fwd == DAU_ALGO_TILED;
    info->gather_patch = tiled_fwd ? top.tiled[kFwd].tiles_x * top.tiled[kFwd].tile_w : 0;
    info->gather_stack = tiled_fwd ? top.tiled[kFwd].stack : 0;
    info->dot_windows = plan->algo_bwd == DAU_ALGO_TILED ? top.tiled_dot.windows : 0;
    info->gather_windows = tiled_fwd ? top.tiled[kFwd].windows : 0;
    info->bucket_sets = plan->dynamic ? plan->nsets : 1;
    // the dense member is bucket 4: reachable as the static set itself, or through the per-call selection
    const bool dense_reachable = s0[kBf16R4] && (plan->nsets == 1 || plan->dynamic);
    info->gather_dense_bf16 = dense_reachable ? (s0[kWgradR4] ? 2 : 1) : 0;
    info->batch_slab_gather = top.slab_gather;
    info->batch_slab_dot = top.slab_dot;
    info->dot_region = top.has[kTiledDot] ? top.tiled_dot.region_cols * 100 + top.tiled_dot.region_rows : 0;
    info->gather_fblock = tiled_fwd ? top.tiled[kFwd].fblock : 0;
    info->gather_variant = tiled_fwd ? top.tiled[kFwd].variant : -1;
    info->dense_bf16_radius3 = dense_reachable && plan->dynamic && s0[kBf16R3] ? (s0[kWgradR3] ? 2 : 1) : 0;
    // the members a call can reach that report themselves: held, per-call selection on, their pass on the tiled kernels
    info->gather_dense_split = plan->sets[0].ring ? 1 << kRingInfoBit : 0;
    const bool tiled_pass[2] = {tiled_fwd, plan->algo_bwd == DAU_ALGO_TILED};   // [PassKind]
    for (int m = 0; m < kNumMembers; ++m)
        if (kMember[m].info_bit >= 0 && s0[m] && plan->dynamic && tiled_pass[kMember[m].kind])
            info->gather_dense_split |= 1 << kMember[m].info_bit;
    return DAU_OK;
}

int dau_conv_split_dot_geometry(const dau_conv_plan* plan, int32_t* region_width, int32_t* strip_items, int32_t* strip_k_steps) {
    if (!plan) return fail(DAU_INVALID_ARGUMENT, "null argument");
    int rw = 0, items = 0, steps = 0;
    for (int i = 0; i < plan->nsets && !rw; ++i) {
        const BucketSet& bs = plan->sets[i];
        if (!bs.has[kSplitDot]) continue;
        const SplitDotConfig& cfg = bs.sdot[kMember[kSplitDot].slot];
        rw = cfg.RW;
        split_dot_strip(cfg, &items, &steps);
    }
    if (region_width) *region_width = rw;
    if (strip_items) *strip_items = items;
    if (strip_k_steps) *strip_k_steps = steps;
    return DAU_OK;
}

int dau_conv_workspace_bytes(const dau_conv_plan* plan, int pass, size_t* bytes_out) {
    if (!plan || !bytes_out) return fail(DAU_INVALID_ARGUMENT, "null argument");
    if (pass == DAU_PASS_FORWARD) *bytes_out = carve_forward(plan, nullptr).bytes;
    else if (pass == DAU_PASS_BACKWARD) *bytes_out = carve_backward(plan, nullptr).bytes;
    else if (pass == DAU_PASS_EPILOGUE_BACKWARD)
        *bytes_out = epilogue_grad_workspace_bytes(plan->sh.N, plan->sh.F, plan->sh.H, plan->sh.W, plan->act(), plan->d.flags & DAU_FLAG_IO_NHWC);
    else return fail(DAU_INVALID_ARGUMENT, "pass must be DAU_PASS_FORWARD, DAU_PASS_BACKWARD or DAU_PASS_EPILOGUE_BACKWARD");
    return DAU_OK;
}

namespace {
int forward_pass(const dau_conv_plan* p, void* stream, const float* x, const float* w, const float* mu1,
                 const float* mu2, const float* sigma, float* y, void* workspace, size_t workspace_bytes, const Epilogue& epi) {
    if (!p || !x || !w || !mu1 || !mu2 || !sigma || !y || !workspace) return fail(DAU_INVALID_ARGUMENT, "null argument");
    FwdWs ws = carve_forward(p, workspace);
    if (workspace_bytes < ws.bytes)
        return fail(DAU_INVALID_ARGUMENT, "workspace too small: %zu < %zu", workspace_bytes, ws.bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ensure_attrs(p)) return rc;
    launch_synth_filters(st, sigma, p->blur_k, p->d.flags, ws.filters, p->host_status, ws.status);
    launch_prepare_units(st, w, mu1, mu2, p->sh, p->d.number_units_ignore, p->d.flags, p->bucket, false, ws.table, ws.status,
                         p->host_status, -1, p->sets[0].has[kLine4] ? ws.status : nullptr);
    run_gather_sum(p, st, kFwd, x, y, ws.filters, ws.table, ws.status, ws.gather, epi);
    DAU_HIP(hipPeekAtLastError());
    return DAU_OK;
}
}  // namespace

int dau_conv_forward(const dau_conv_plan* p, void* stream, const float* x, const float* w, const float* mu1,
                     const float* mu2, const float* sigma, float* y, void* workspace, size_t workspace_bytes) {
    return forward_pass(p, stream, x, w, mu1, mu2, sigma, y, workspace, workspace_bytes, Epilogue{});
}

namespace {
// whether the plan's forward pass takes a fused `what` (an epilogue, a residual); bf16_has: what the bf16-product forms have of it
int fused_store_supported(const dau_conv_plan* p, int epilogue, const char* what, const char* bf16_has) {
    if (!p) return fail(DAU_INVALID_ARGUMENT, "null argument");
    if (epilogue & ~(DAU_EPILOGUE_BIAS | DAU_EPILOGUE_RELU))
        return fail(DAU_INVALID_ARGUMENT, "unknown epilogue bits 0x%x (DAU_EPILOGUE_BIAS | DAU_EPILOGUE_RELU)", epilogue);
    if (p->algo_fwd != DAU_ALGO_TILED)
        return fail(DAU_INVALID_ARGUMENT, "the direct kernels take no fused %s (this plan's forward pass runs on them)", what);
    if (p->d.flags & DAU_FLAG_DENSE_BF16)
        return fail(DAU_INVALID_ARGUMENT, "DAU_FLAG_DENSE_BF16 plans take no fused %s (the bf16-product forms have %s)", what, bf16_has);
    return DAU_OK;
}
}  // namespace

int dau_conv_epilogue_supported(const dau_conv_plan* p, int epilogue) { return fused_store_supported(p, epilogue, "epilogue", "none"); }

int dau_conv_forward_residual(const dau_conv_plan* p, void* stream, const float* x, const float* w, const float* mu1,
                              const float* mu2, const float* sigma, const float* bias, const float* residual, int epilogue,
                              float* y, void* workspace, size_t workspace_bytes) {
    Epilogue epi;
    if (residual || epilogue) {
        // the residual is no epilogue bit: it is taken where a bias is (dau_conv_epilogue_supported(p, DAU_EPILOGUE_BIAS)), also with epilogue == 0
        if (int rc = residual ? fused_store_supported(p, epilogue, "residual", "no epilogue") : dau_conv_epilogue_supported(p, epilogue)) return rc;
        if ((epilogue & DAU_EPILOGUE_BIAS) && !bias) return fail(DAU_INVALID_ARGUMENT, "DAU_EPILOGUE_BIAS without a bias");
        epi.bias = (epilogue & DAU_EPILOGUE_BIAS) ? bias : nullptr;
        epi.relu = (epilogue & DAU_EPILOGUE_RELU) != 0;
        epi.residual = residual;
    }
    return forward_pass(p, stream, x, w, mu1, mu2, sigma, y, workspace, workspace_bytes, epi);
}

int dau_conv_forward_epilogue(const dau_conv_plan* p, void* stream, const float* x, const float* w, const float* mu1,
                              const float* mu2, const float* sigma, const float* bias, int epilogue, float* y,
                              void* workspace, size_t workspace_bytes) {
    return dau_conv_forward_residual(p, stream, x, w, mu1, mu2, sigma, bias, nullptr, epilogue, y, workspace, workspace_bytes);
}

int dau_conv_epilogue_backward(const dau_conv_plan* p, void* stream, const float* dy, const float* y, int epilogue, float* dz,
                               float* dbias, void* workspace, size_t workspace_bytes) {
    if (!p || !dy) return fail(DAU_INVALID_ARGUMENT, "null argument");
    if (epilogue & ~(DAU_EPILOGUE_BIAS | DAU_EPILOGUE_RELU))
        return fail(DAU_INVALID_ARGUMENT, "unknown epilogue bits 0x%x (DAU_EPILOGUE_BIAS | DAU_EPILOGUE_RELU)", epilogue);
    const bool relu = (epilogue & DAU_EPILOGUE_RELU) != 0;
    if (!(epilogue & DAU_EPILOGUE_BIAS)) dbias = nullptr;     // the bits select the work: no bias, no sum
    if (relu && (!y || !dz)) return fail(DAU_INVALID_ARGUMENT, "DAU_EPILOGUE_RELU needs y and dz");
    const bool nhwc = (p->d.flags & DAU_FLAG_IO_NHWC) != 0;
    const Shape& s = p->sh;
    if (dbias) {
        const size_t need = epilogue_grad_workspace_bytes(s.N, s.F, s.H, s.W, p->act(), nhwc);
        if (!workspace || workspace_bytes < need)
            return fail(DAU_INVALID_ARGUMENT, "workspace too small: %zu < %zu", workspace ? workspace_bytes : (size_t)0, need);
    }
    if (!epilogue_grad_run(static_cast<hipStream_t>(stream), s.N, s.F, s.H, s.W, p->act(), nhwc, dy, y, relu, dz, dbias, workspace))
        return fail(DAU_INVALID_ARGUMENT, "activation tensor too large for the epilogue's backward pass");
    DAU_HIP(hipPeekAtLastError());
    return DAU_OK;
}

namespace {

// raw parameter-gradient sums r4[k][s][g][f] = offset_and_dot(x * D_k, dy') with bare bilinear factors
// kinds: 4, or 3 when the caller does not want dsigma (only the dense form computes fewer: its GEMMs are per kind)
// w: the weights where the caller has them (dau_conv_backward), for the line members' count alone; the table is bare either way
int run_param_sums(const dau_conv_plan* p, hipStream_t st, const float* x, const float* dy, const float* mu1,
                   const float* mu2, const BwdWs& ws, float* r4, int kinds, const float* w = nullptr) {
    const Shape& s = p->sh;
    // (the gather-dot's line members: their condition is counted on THIS table, into Status::dot_off_line_units for the report and
    // into off_line_units, which the guards read; off_line_units goes back to zero behind the pass, for the count of the
    // input-gradient table; a NaN / Inf weight counts where the caller has the weights)
    const bool dot_line = p->algo_bwd == DAU_ALGO_TILED && p->dynamic && p->sets[0].has[kDotLine4];
    launch_prepare_units(st, dot_line ? w : nullptr, mu1, mu2, s, p->d.number_units_ignore, p->d.flags, p->bucket, false, ws.table_bare,
                         ws.status, p->host_status, -1, dot_line ? ws.status : nullptr, true);
    if (p->profiling) ++p->prof_passes[2];
    if (p->algo_bwd == DAU_ALGO_TILED) {
        Candidate cand[kMaxCandidates];
        const int ncand = pick_candidates(p, ws.status, kGatherDot, cand);
        for (int ci = 0; ci < ncand; ++ci) {
            const BucketSet& bs = *cand[ci].set;
            const Guard& g = cand[ci].guard;
            const int m = cand[ci].member;
            const int slot = kMember[m].slot;
            if (kMember[m].family == kFamSplitDot) {                           // the whole batch in one pass
                const SplitDotFns& fn = kSplitDotFns[slot];
                fn.prepare(st, bs.sdot[slot], x, dy, ws.filters, p->drop_col, p->drop_row, ws.tiled_dot, g);
                ProfScope prof(p, 2, st);
                fn.run(st, bs.sdot[slot], ws.table_bare, r4, ws.tiled_dot, g);
            } else if (kMember[m].family == kFamWgrad) {                       // likewise
                ProfScope prof(p, 2, st);
                kWgrad[slot].run(st, bs.wgrad[slot], x, dy, ws.filters, ws.table_bare, p->drop_col, p->drop_row, r4, ws.tiled_dot, g, kinds);
            } else {
                for (int n0 = 0; n0 < s.N; n0 += bs.slab_dot) {            // the sums of the slabs add up in r4
                    tiled_dot_prepare(st, bs.tiled_dot, slab_ptr(x, (size_t)n0 * s.S * s.H * s.W, p->esize()),
                                      slab_ptr(dy, (size_t)n0 * s.F * s.H * s.W, p->esize()), ws.filters, ws.table_bare,
                                      p->drop_col, p->drop_row, ws.tiled_dot, g);
                    ProfScope prof(p, 2, st);
                    tiled_dot_run(st, bs.tiled_dot, r4, ws.tiled_dot, g, n0 > 0);
                }
            }
        }
        if (dot_line) launch_zero_words(st, &ws.status->off_line_units, sizeof(unsigned));
    } else {
        launch_blur_direct(st, x, (long)s.N * s.S, s.H, s.W, ws.filters + 1 * kFilterPlane, kNumK, p->blur_k, ws.xk4);
        ProfScope prof(p, 2, st);
        launch_gather_dot_direct(st, ws.xk4, dy, ws.table_bare, s, p->drop_col, p->drop_row, r4);
    }
    return DAU_OK;
}

int check_backward_ws(const dau_conv_plan* p, void* workspace, size_t workspace_bytes, BwdWs* ws) {
    *ws = carve_backward(p, workspace);
    if (workspace_bytes < ws->bytes)
        return fail(DAU_INVALID_ARGUMENT, "workspace too small: %zu < %zu", workspace_bytes, ws->bytes);
    return DAU_OK;
}

}  // namespace

int dau_conv_backward(const dau_conv_plan* p, void* stream, const float* x, const float* dy, const float* w,
                      const float* mu1, const float* mu2, const float* sigma, float* dx, float* dw, float* dmu1,
                      float* dmu2, float* dsigma, void* workspace, size_t workspace_bytes, int need_mask) {
    // (x: the parameter gradients read it; so does the dx pass of a DAU_FLAG_INPUT_RELU plan, as its mask)
    if (p && !x && (p->d.flags & DAU_FLAG_INPUT_RELU) && (need_mask & DAU_NEED_DX))
        return fail(DAU_INVALID_ARGUMENT, "DAU_FLAG_INPUT_RELU: the input-gradient pass masks dx by x, which is null");
    if (!p || !x || !dy || !w || !mu1 || !mu2 || !sigma || !workspace) return fail(DAU_INVALID_ARGUMENT, "null argument");
    if (((need_mask & DAU_NEED_DX) && !dx) || ((need_mask & DAU_NEED_DW) && !dw) ||
        ((need_mask & DAU_NEED_DMU1) && !dmu1) || ((need_mask & DAU_NEED_DMU2) && !dmu2) ||
        ((need_mask & DAU_NEED_DSIGMA) && !dsigma))
        return fail(DAU_INVALID_ARGUMENT, "need_mask asks for a gradient whose output pointer is null");
    BwdWs ws;
    if (int rc = check_backward_ws(p, workspace, workspace_bytes, &ws)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Shape& s = p->sh;
    const int flags = p->d.flags;
    if (int rc = ensure_attrs(p)) return rc;
    launch_synth_filters(st, sigma, p->blur_k, flags, ws.filters, p->host_status, ws.status);

    const int param_mask = DAU_NEED_DW | DAU_NEED_DMU1 | DAU_NEED_DMU2 | DAU_NEED_DSIGMA;
    if (need_mask & param_mask) {
        run_param_sums(p, st, x, dy, mu1, mu2, ws, ws.r4, (need_mask & DAU_NEED_DSIGMA) ? 4 : 3, w);
        launch_finalize_grads(st, ws.r4, w, s, p->d.number_units_ignore, p->d.mu_learning_rate_factor, need_mask,
                              flags & DAU_FLAG_SINGLE_DIM_KERNEL, dw, dmu1, dmu2, dsigma);
    }
    if (need_mask & DAU_NEED_DX) {
        // input gradient: the forward gather on the mirrored-Gaussian-blurred error with the
        // parameters read as [F,G,S] and negated offsets (base_dau_conv_layer.cu:299-325)
        const bool fresh = !(need_mask & param_mask);     // this call has not looked at the offsets yet
        // (the line members' condition is counted on THIS table, whether or not the offsets have been looked at)
        launch_prepare_units(st, w, mu1, mu2, s, 0, flags, p->bucket, true, ws.table_t, fresh ? ws.status : nullptr,
                             p->host_status, p->d.number_units_ignore, p->sets[0].has[kLine4] ? ws.status : nullptr);
        // DAU_FLAG_INPUT_RELU: the ReLU's backward in the store, dx = (x <= 0) ? 0 : sum, from the raw x at the store's own index
        Epilogue gate;
        if (flags & DAU_FLAG_INPUT_RELU) gate.gate = x;
        run_gather_sum(p, st, kDx, dy, dx, ws.filters, ws.table_t, ws.status, ws.gather_dx, gate);
    }
    DAU_HIP(hipPeekAtLastError());
    return DAU_OK;
}

int dau_conv_backward_param_sums(const dau_conv_plan* p, void* stream, const float* x, const float* dy, const float* mu1,
                                 const float* mu2, const float* sigma, float* sums_out, void* workspace,
                                 size_t workspace_bytes) {
    if (!p || !x || !dy || !mu1 || !mu2 || !sigma || !sums_out || !workspace) return fail(DAU_INVALID_ARGUMENT, "null argument");
    BwdWs ws;
    if (int rc = check_backward_ws(p, workspace, workspace_bytes, &ws)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ensure_attrs(p)) return rc;
    launch_synth_filters(st, sigma, p->blur_k, p->d.flags, ws.filters, p->host_status, ws.status);
    run_param_sums(p, st, x, dy, mu1, mu2, ws, sums_out, 4);
    DAU_HIP(hipPeekAtLastError());
    return DAU_OK;
}

int dau_conv_finalize_param_grads(const dau_conv_plan* p, void* stream, const float* sums, const float* w, float* dw,
                                  float* dmu1, float* dmu2, float* dsigma, int need_mask) {
    if (!p || !sums || !w) return fail(DAU_INVALID_ARGUMENT, "null argument");
    if (((need_mask & DAU_NEED_DW) && !dw) || ((need_mask & DAU_NEED_DMU1) && !dmu1) ||
        ((need_mask & DAU_NEED_DMU2) && !dmu2) || ((need_mask & DAU_NEED_DSIGMA) && !dsigma))
        return fail(DAU_INVALID_ARGUMENT, "need_mask asks for a gradient whose output pointer is null");
    launch_finalize_grads(static_cast<hipStream_t>(stream), sums, w, p->sh, p->d.number_units_ignore,
                          p->d.mu_learning_rate_factor, need_mask, p->d.flags & DAU_FLAG_SINGLE_DIM_KERNEL, dw, dmu1, dmu2,
                          dsigma);
    DAU_HIP(hipPeekAtLastError());
    return DAU_OK;
}

namespace {
// the status block of the last call on `workspace`, once the stream has run it
int read_status(const dau_conv_plan* p, void* stream, const void* workspace, Status* h) {
    if (!p || !workspace) return fail(DAU_INVALID_ARGUMENT, "null argument");
    DAU_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    DAU_HIP(hipMemcpy(h, workspace, sizeof(Status), hipMemcpyDeviceToHost));
    return DAU_OK;
}
}  // namespace

int dau_conv_check_status(const dau_conv_plan* p, void* stream, const void* workspace, float* max_abs_mu_out) {
    Status h;
    if (int rc = read_status(p, stream, workspace, &h)) return rc;
    float mx;
    std::memcpy(&mx, &h.max_abs_mu_bits, sizeof(float));
    if (max_abs_mu_out) *max_abs_mu_out = mx;
    if (h.nan_seen || mx > (float)p->bucket) clear_reported_status(p, h.max_abs_mu_bits, h.nan_seen != 0);   // reported here
    return status_error(p, mx, h.nan_seen != 0);
}

int dau_conv_gather_outlier_status(const dau_conv_plan* p, void* stream, const void* workspace, int32_t* outlier_units,
                                   int32_t* ring_taken) {
    Status h;
    if (int rc = read_status(p, stream, workspace, &h)) return rc;
    if (outlier_units) *outlier_units = (int32_t)(h.outlier_units & ~kRingTakenBit);
    if (ring_taken) *ring_taken = (h.outlier_units & kRingTakenBit) ? 1 : 0;
    return DAU_OK;
}

int dau_conv_gather_line_status(const dau_conv_plan* p, void* stream, const void* workspace, int32_t* off_line_units,
                                int32_t* line_radius_taken) {
    Status h;
    if (int rc = read_status(p, stream, workspace, &h)) return rc;
    if (off_line_units) *off_line_units = (int32_t)h.off_line_units;
    if (line_radius_taken) *line_radius_taken = (int32_t)h.line_radius;
    return DAU_OK;
}

int dau_conv_dot_line_status(const dau_conv_plan* p, void* stream, const void* workspace, int32_t* off_line_units,
                             int32_t* line_radius_taken) {
    Status h;
    if (int rc = read_status(p, stream, workspace, &h)) return rc;
    if (off_line_units) *off_line_units = (int32_t)h.dot_off_line_units;
    if (line_radius_taken) *line_radius_taken = (int32_t)h.dot_line_radius;
    return DAU_OK;
}

int dau_conv_last_status(const dau_conv_plan* p, float* max_abs_mu_out, int32_t* valid_out) {
    if (!p) return fail(DAU_INVALID_ARGUMENT, "null argument");
    if (max_abs_mu_out) *max_abs_mu_out = 0.0f;
    if (valid_out) *valid_out = 0;
    if (!p->host_status) return DAU_OK;
    const volatile HostStatus* h = p->host_status;
    if (h->valid != 1u && h->bad_max_abs_mu_bits == 0u && h->bad_nan_seen == 0u) return DAU_OK;   // no call has completed yet
    // the sticky record first: the worst status of ANY completed call since the last report (a later good call of another
    // layer sharing this plan must not hide it); then the most recent call
    const unsigned bad_bits = h->bad_max_abs_mu_bits, bad_nan = h->bad_nan_seen;
    unsigned bits = h->max_abs_mu_bits, nan_seen = h->nan_seen | bad_nan;
    if (bad_bits > bits) bits = bad_bits;                // non-negative float bits order like unsigned integers
    float mx;
    std::memcpy(&mx, &bits, sizeof(float));
    if (max_abs_mu_out) *max_abs_mu_out = mx;
    if (valid_out) *valid_out = 1;
    // a bad status is reported once: the mirror goes back to "nothing reported" until the next call completes
    if (nan_seen || mx > (float)p->bucket) clear_host_status(p);
    return status_error(p, mx, nan_seen != 0);
}

int dau_conv_sigma_status(const dau_conv_plan* p, int32_t* needed_out, int32_t* planned_out, int32_t* worst_needed_out) {
    if (!p || !needed_out || !planned_out || !worst_needed_out) return fail(DAU_INVALID_ARGUMENT, "null argument");
    *needed_out = 0;
    *planned_out = p->blur_k;
    *worst_needed_out = 0;
    if (!p->host_status) return DAU_OK;                  // no device: no call can have run
    volatile HostStatus* h = p->host_status;
    *needed_out = (int32_t)h->sigma_needed;
    *worst_needed_out = (int32_t)h->sigma_worst;
    h->sigma_worst = 0u;                                 // reported: sticky until here
    return DAU_OK;
}

int dau_conv_filters(const dau_conv_plan* p, void* stream, const float* sigma, float* filters_out) {
    if (!p || !sigma || !filters_out) return fail(DAU_INVALID_ARGUMENT, "null argument");
    // the six k x k planes are written straight into the caller's buffer: no scratch, no sync
    launch_synth_filters_compact(static_cast<hipStream_t>(stream), sigma, p->blur_k, p->d.flags, filters_out);
    DAU_HIP(hipPeekAtLastError());
    return DAU_OK;
}

int dau_conv_unit_table(const dau_conv_plan* p, void* stream, const float* w, const float* mu1, const float* mu2, int form,
                        void* table_out) {
    if (!p || !mu1 || !mu2 || !table_out) return fail(DAU_INVALID_ARGUMENT, "null argument");
    if (form != 0 && form != 1) return fail(DAU_INVALID_ARGUMENT, "form must be 0 ([S][G][F]) or 1 ([F][G][S], negated offsets)");
    // the kernel every forward / backward call runs first, writing into the caller's buffer instead of the workspace
    // (the input-gradient pass ignores no unit: the reference transposes the ignored units' zero weights along)
    launch_prepare_units(static_cast<hipStream_t>(stream), w, mu1, mu2, p->sh, form == 1 ? 0 : p->d.number_units_ignore, p->d.flags,
                         p->bucket, form == 1, static_cast<UnitRef*>(table_out), nullptr, nullptr);
    DAU_HIP(hipPeekAtLastError());
    return DAU_OK;
}

}  // extern "C"
