// libzip_hip.so -- C ABI (include/zip_hip.h) over the gfx950 kernels.
// Host-side runtime: context / stream ownership, a caching device allocator (so a
// commit of several GiB does not pay hipMalloc/hipFree per call), geometry
// validation mirroring the reference's error behaviour, kernel dispatch and the
// HIP-event measurement hooks used by bench.py.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/zip_hip.h"
#include "kernels_commit.cuh"
#include "kernels_open.cuh"
#include "kernels_batch.cuh"
#include "kernels_verify.cuh"
#include "kernels_batch_verify.cuh"
#include "kernels_sumcheck.cuh"
#include "kernels_sumcheck_tail.cuh"
#include "kernels_sumcheck_batch.cuh"
#include "kernels_sumcheck_wide.cuh"
#include "kernels_sumcheck_products.cuh"
#include "kernels_spartan.cuh"
#include "kernels_spartan_batch.cuh"
#include "kernels_prime.cuh"
#include "kernels_prime_batch.cuh"
#include "kernels_two_limb.cuh"
#include "rccl_dyn.h"

using namespace zipk;

namespace {

typedef unsigned __int128 u128;

// ------------------------------------------------------------------ small utils
bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }
uint32_t ilog2(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }

// An integer knob from the environment: `def` when it is unset, not a number or outside [lo, hi].
long env_long(const char *name, long def, long lo, long hi) {
    const char *e = getenv(name);
    if (!e) return def;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    return end == e || v < lo || v > hi ? def : v;
}

struct KernelStat {
    uint32_t launches = 0;
    float total_ms = 0.f;
};
struct PendingEvent {
    const char *name;
    hipEvent_t start, stop;
};

// What FieldConfig::new makes of a modulus (make_field): the context's memo, and the field of a sumcheck / CCS handle
struct HostField {
    uint32_t fl = 0;
    uint64_t modulus[8]{}, r[8]{}, r2[8]{};
    uint64_t inv = 0;
    uint64_t quirk_mod = 0;
};

}  // namespace

// (documented with get_hint_plan below)
struct PackedLayout {
    uint32_t stride = 0, off[3] = {};
};
struct HintPlan {
    uint32_t cw = 0, e = 0, threads = 0;
    bool want_packed = false;
    std::vector<uint32_t> cols;
    std::vector<uint32_t> bm;
    bool packed = false;
    PackedLayout L;
    // CommitArgs.pk_tab: e = 16: [waves][phases][16] words = 32 16-bit bases each; e = 8: [threads][2] words = the
    // lane's four 16-bit base ranks (values | N0 << 16, N1 | N2 << 16)
    std::vector<uint32_t> rank_tab;
    std::vector<uint16_t> pos[4];    // 0xFFFF: not a member
    std::vector<uint16_t> own_ranks; // pk_rank of cols[] themselves, [n][4] (OpenColsArgs.pk_rank)
    // device copy, made once: bm at 0 (CommitArgs.need), rank_tab at kHintTables, own_ranks at kPackedRanksAt
    unsigned char *dev = nullptr;
    std::function<void(unsigned char *)> release;  // gives `dev` back to its ctx's block pool (hipFree would stall the device)
    HintPlan() = default;
    HintPlan(const HintPlan &) = delete;
    HintPlan &operator=(const HintPlan &) = delete;
    ~HintPlan() { if (dev && release) release(dev); }
    // pk_rank of cs[i]: place of its value and of its three lowest siblings
    bool ranks(const uint32_t *cs, uint32_t n, uint16_t *out) const {
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t col = cs[i];
            if (col >= cw) return false;
            const uint16_t r[4] = {pos[0][col], pos[1][col ^ 1u], pos[2][(col >> 1) ^ 1u], pos[3][(col >> 2) ^ 1u]};
            for (int k = 0; k < 4; k++) {
                if (r[k] == 0xFFFF) return false;
                out[4 * i + k] = r[k];
            }
        }
        return true;
    }
};

// zip_ctx::speculate: 0 = never, 1 = only where the library owns a copy of the witness (HOST witnesses: the default --
// nothing about the caller's buffers changes), 2 = DEVICE witnesses too (opt-in, zip_ctx_set_speculation(ctx, 1): the
// caller then keeps its device witness valid and unchanged until the handle is freed).  ZIP_HIP_SPECULATE=0 / 1
// sets the process-wide default to 0 / 2.
static inline int speculation_default_flag() {
    const long v = env_long("ZIP_HIP_SPECULATE", -1, 0, 1);
    return v < 0 ? 1 : v == 0 ? 0 : 2;
}

struct zip_ctx {
    zip_params p{};
    uint32_t depth = 0;
    uint32_t rows_local = 0;
    // LinearCodeSpec::num_proximity_testing (zip_ctx_set_proximity_tests): proximity rows the single-context open and
    // verify paths write and check.  1 launches exactly what a ctx without the notion launched.
    uint32_t n_tests = 1;
    int device = 0;
    // Three HIP streams form a row-chunked pipeline: `s_commit` runs the fused
    // encode+hash kernel chunk by chunk, `s_upper` the upper Merkle levels of each finished
    // chunk, and `stream` everything else (row combinations, column openings, copies).  Per-chunk
    // events let the memory-bound column gather of chunk k overlap the VALU-bound hashing of
    // chunk k+1.
    hipStream_t stream = nullptr, s_commit = nullptr, s_upper = nullptr;
    uint32_t n_chunks = 1;
    // knobs read from the environment ONCE, by zip_ctx_create (the calls read none of them again): ZIP_HIP_GATHER_RPB
    // (0: unset), ZIP_HIP_GATHER_STREAM (-1: unset), ZIP_HIP_CHUNK_ROUNDS (empty: unset), ZIP_HIP_NO_COMPACT_ROWS
    uint32_t knob_rpb = 0;
    int knob_stream = -1;
    std::string knob_chunk_rounds;
    bool no_compact = false;
    uint32_t num_cus = 256;
    uint32_t *timeout_flag_h = nullptr, *timeout_flag_d = nullptr;  // pinned: a pipeline wait gave up
    unsigned long long *clock_h = nullptr, *clock_d = nullptr;      // pinned: CommitArgs.clock stamps of the last profiled commit
    std::vector<hipEvent_t> dep_event_pool;  // hipEventDisableTiming
    uint32_t *perm1_d = nullptr, *perm2_d = nullptr;
    // pinned host staging for the small per-call inputs (coeffs, q0, column indices): one
    // truly asynchronous H2D copy instead of several pageable (blocking, staged) ones
    unsigned char *pinned_base = nullptr, *stage_h = nullptr, *stage_big = nullptr;
    size_t stage_cap = 0, stage_big_cap = 0;
    // zip_open_stream: two pinned bounce buffers the proof leaves the device through
    unsigned char *bounce[2] = {nullptr, nullptr};
    size_t bounce_cap = 0;
    std::vector<unsigned char *> hint_free;  // pinned kHintBytes blocks of dead hinted commitments
    std::shared_ptr<bool> alive = std::make_shared<bool>(true);  // false once zip_ctx_destroy has run
    bool profile_commit_only = false;  // zip_ctx_set_profiling(ctx, 2)
    std::shared_ptr<HintPlan> hint_plan;  // what the last hinted commit derived from its column list (memo)
    int speculate = speculation_default_flag();   // zip_commit hints itself with the columns of the ctx's last opening (0 / 1 / 2, above)
    bool seen_columns = false;                    // ... once an opening (or an explicit hint) has named some
    // chunk arrival counters of the persistent commit kernel: kRingSlots zeroed blocks of kRingStride counters, handed
    // out in turn; every kRingSlots commits the ring is zeroed again (ring_epoch moves: an older handle's counters
    // are gone, its openings then wait for the whole commit instead)
    uint32_t *ring_d = nullptr;
    uint32_t ring_next = 0, ring_epoch = 0;
    // raa_commit_slab_kernel (cw 32768 / 65536): one slab of cw 16-byte entries per workgroup (CommitArgs.slab),
    // allocated at the first such commit; every commit kernel of the ctx runs on s_commit, one after the other
    uint4 *slab_d = nullptr;
    size_t slab_bytes = 0;
    // zip_commit_open_begin: pinned staging of the jobs in flight (kJobSlots), and which slots are taken
    unsigned char *job_stage[2] = {nullptr, nullptr};
    size_t job_stage_cap[2] = {0, 0};  // bytes of job_stage[slot] (job_stage_bytes: grows with the rows and the field)
    bool job_busy[2] = {false, false};
    // bumped by every recovery from a timed-out pipeline wait (recover_gather_timeout).  A job enqueued BEFORE a recovery
    // that another job ran cannot tell any more whether its own waits gave up too (the flag is cleared): it re-gathers.
    // Jobs enqueued after it are covered by the flag again.
    uint64_t recover_epoch = 0;
    // make_field memo: the last zip_field seen and what FieldConfig::new made of it
    zip_field field_cache_in{};
    HostField field_cache_out;
    bool field_cache_valid = false;
    std::string last_error;
    // private plumbing context of a zip_sumcheck / zip_ccs: its blocks go to the process-wide recycle bin
    // when it dies and are taken from there first (these handles live for one proof, hipMalloc is ~ms)
    bool recycle = false;
    size_t h2d_bounce_threshold = (size_t)8 << 20;  // below: plain hipMemcpyAsync from the caller's (pageable) memory
    // caching allocator: exact-size free lists
    std::multimap<size_t, void *> free_blocks;
    std::map<void *, size_t> live_blocks;
    std::mutex mu;
    // Serialises the exported calls on this ctx (and on its commitments): they share one pinned
    // staging buffer and one set of streams.  Distinct contexts run concurrently.
    std::recursive_mutex api_mu;
    // measurement
    bool profiling = false;
    std::vector<PendingEvent> pending;
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, KernelStat> stats;
    std::vector<std::string> stat_names;  // stable storage for returned names
};

// The device storage of a zip_batch: the row entries, trees and roots of all its polynomials in one block each (and the
// library's copy of a HOST witness; for zip_batch_commit_codes the members' permutations, perm1 slices then perm2
// slices).  The batch and every member handle taken from it (zip_batch_member) hold a reference; the blocks return to
// the pool with the last of them.
struct BatchStore {
    void *rows = nullptr, *layers = nullptr, *roots = nullptr, *evals = nullptr, *perms = nullptr;
    std::function<void(BatchStore &)> release;
    BatchStore() = default;
    BatchStore(const BatchStore &) = delete;
    BatchStore &operator=(const BatchStore &) = delete;
    ~BatchStore() { if (release) release(*this); }
};

struct zip_batch {
    zip_ctx *ctx = nullptr;
    uint32_t n_polys = 0;
    std::shared_ptr<BatchStore> store;
    const int64_t *evals_d = nullptr;  // [n_polys][num_rows][row_len] on the device: the store's copy, or the caller's array
};

struct zip_commitment {
    // a member of a zip_batch: rows / layers / roots / evals point INTO the batch's blocks (`store` keeps them alive)
    // and are not this handle's to release -- except `rows` once materialize_rows has replaced them by a copy
    std::shared_ptr<BatchStore> store;
    bool borrows_rows = false, borrows_rest = false;
    const uint32_t *gather_order = nullptr;  // device, valid during one open: OpenColsArgs.order
    zip_ctx *ctx = nullptr;
    uint64_t *rows = nullptr;   // [rows_local][cw][4], or [rows_local][cw][2] while compact_rows (see materialize_rows)
    bool compact_rows = false;
    uint32_t *layers = nullptr;  // [rows_local][2cw][8] or null (commit_no_merkle)
    uint32_t *roots = nullptr;   // [rows_local][8] or null
    int64_t *evals = nullptr;    // device copy owned by the handle when the witness came from the host
    size_t rows_bytes = 0, layers_bytes = 0, roots_bytes = 0, evals_bytes = 0;
    // Pipeline state of the persistent commit kernel that produces this handle: chunk k = rows
    // [bounds[k], bounds[k+1]) is complete (rows, trees, roots) once chunk_done[k] == expected[k].
    std::vector<uint32_t> bounds, expected;
    uint32_t *chunk_done = nullptr;  // device arrival counters (a pool block, or a slot of the ctx's ring)
    const uint4 *gather_tab = nullptr;  // device, valid during one open: OpenColsArgs.wg_tab (packed handles)
    bool ring_slot = false;
    uint32_t ring_epoch = 0;
    bool consumers_done = false;  // set by zip_job_wait: nothing on the ctx's streams still reads this handle
    hipEvent_t zeroed = nullptr;     // counters reset (consumers must not look at stale values)
    hipEvent_t done = nullptr;       // whole commit finished
    std::vector<hipEvent_t> aux;     // other events owned by the handle, recycled with it
    // zip_commit_hinted: the kernel only stored what an opening of the hinted columns reads.  `hint_cols` is the
    // set (bit c = column c was hinted); anything else asked of the handle first re-runs the commit in full
    // (rematerialize) from the witness: `evals` above, or the caller's device array `evals_ref`.
    bool hinted = false;
    // zip_commit_open, packed openings: values and level-0..2 nodes of the hinted columns sit densely in `rows`
    // (CommitArgs.pk), at the positions `plan` holds
    bool packed = false;
    uint32_t pk_stride = 0, pk_off[3] = {};
    std::shared_ptr<HintPlan> plan;  // bitmaps, packed layout and the position of every member (HintPlan)
    const uint16_t *rank_d = nullptr;  // device (inside need_d): OpenColsArgs.pk_rank of the hinted openings, in their order
    std::vector<uint32_t> hint_cols;
    unsigned char *hint_h = nullptr;  // pinned staging of the bitmaps (returns to ctx->hint_free)
    uint32_t *need_d = nullptr;       // device bitmaps (CommitArgs.need)
    const int64_t *evals_ref = nullptr;
    // zip_commit's SPECULATIVE hint (the ctx's last column list): the caller never promised to keep a DEVICE witness
    // unchanged, so its digest is taken beside the commit kernel and checked before a re-run reads evals_ref again
    bool speculative = false;
    unsigned long long *digest_d = nullptr;  // [2], pool block
    hipEvent_t digest_done = nullptr;
    CommitArgs args{};                // the launch, for the re-run
    uint32_t grid = 0;
};

// Prover state of one sumcheck (ProverState, src/sumcheck/prover.rs:25-37) on the device.
struct zip_sumcheck {
    zip_ctx *ctx = nullptr;  // private plumbing context (stream, pool, error text)
    uint32_t n_mles = 0, num_vars = 0, degree = 0, fl = 0, round = 0;
    bool pending = false;  // a round has been enqueued (zip_sumcheck_round_begin) and not yet collected
    bool proved = false;   // zip_sumcheck_prove has run: the handle is finished
    uint64_t *tail_out_d = nullptr;  // what sumcheck_tail_kernel writes out (kTailOutBytes)
    const uint64_t *input[kSumcheckProductsMaxMles] = {};  // the tables of round 1 (device; owned when `owned`)
    bool owned = false;
    uint64_t *buf[2][kSumcheckProductsMaxMles] = {};  // ping-pong fold targets: 2^(nv-1) and 2^(nv-2) entries
    uint64_t *partials = nullptr, *evals_d = nullptr;
    uint32_t *done_d = nullptr;          // arrival counter of the round kernel
    unsigned char *evals_pinned = nullptr;  // host-mapped slot the round message is written to (or null: evals_d + a copy)
    uint32_t max_blocks = 0;
    HostField field;  // modulus and Montgomery constants, computed once (512 modular doublings)
    uint32_t n_terms = 0, term_mask[8] = {};  // zip_sumcheck_comb, or n_terms == 0 for the plain product
    uint64_t coeff[8][8] = {};
    // zip_sumcheck_init_products: comb_fn = sum_t coeff[t] * prod_{j in term_mask[t]} vals[j], no trailing factor
    // (sumcheck_round_products_kernel).  n_factors / factors / own: SumcheckProductsArgs.
    bool products = false;
    uint32_t n_factors[8] = {}, factors[8] = {}, own[8] = {};
};

// CCS matrices and the per-proof tables of SpartanProver::prove (src/zinc/prover.rs:130-161) in HBM.
struct zip_ccs {
    zip_ctx *ctx = nullptr;  // private plumbing context (stream, pool, error text)
    uint32_t t = 0, s = 0, m = 0, fl = 0;
    HostField field;
    struct Mat {
        uint32_t n_rows = 0, nnz = 0;
        uint32_t *row_ptr = nullptr, *col_idx = nullptr, *col_ptr = nullptr, *row_idx = nullptr;
        uint64_t *vals = nullptr, *vals_t = nullptr;  // Montgomery: CSR order / CSC order
    } mat[kCcsMaxMatrices];
    uint64_t *z_f = nullptr, *mz[kCcsMaxMatrices] = {}, *eq[2] = {}, *second = nullptr;
    uint64_t *small_d = nullptr, *partials = nullptr;  // challenges in; dot-product partials
    uint64_t *eq_half = nullptr;                       // eq tables over the low / high half of the variables
    uint32_t dot_blocks = 0;
    bool have_z = false, have_eq[2] = {false, false}, have_second = false;
};

// The CCS matrices once, as integers, and the Spartan tables of up to `capacity` proofs of that circuit, each with its
// own field (kernels_spartan_batch.cuh).
struct zip_ccs_batch {
    zip_ctx *ctx = nullptr;  // private plumbing context (stream, pool, error text)
    uint32_t t = 0, s = 0, m = 0, fl = 0, capacity = 0;
    CcsBatchMats mats{};     // device pointers: CSR as uploaded, CSC built once at creation; int64 values in both
    uint64_t *tables = nullptr;  // capacity * (t + 4) tables of m elements: per instance z_f, mz[0..t), eq[0], eq[1], second
    int64_t *z_d = nullptr;      // the z vectors of a HOST set_z, one after the other (capacity * m entries)
    void *args_d = nullptr;      // n CcsBatchInst<fl>; zip_ccs_batch_eval_matrices: then every r_x, then every r_y
    uint64_t *chal_d = nullptr;  // capacity * (s + 1) elements: r of eq_tables, or r_x followed by every gamma
    uint64_t *vs_d = nullptr;    // capacity * t elements
    // what the asynchronous uploads read: kept until the stream has passed them (the next call that refills them waits)
    std::vector<unsigned char> args_h;
    std::vector<int64_t> z_h;
    std::vector<uint64_t> chal_h;
    uint32_t n = 0;  // instances of the last set_z; 0: none yet
    bool have_eq[2] = {false, false}, have_second = false;
    bool in_flight = false;  // work enqueued since the last wait: zip_ccs_batch_table waits before it hands a pointer out
};

namespace {

int32_t fail(zip_ctx *ctx, int32_t code, const char *fmt, ...) {
    if (ctx) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        ctx->last_error = buf;
    }
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(ctx, ZIP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

// Host waits.  A blocked hipStreamSynchronize is woken by an interrupt 20-40 us after the stream has drained -- 1.5 %
// of a 2 ms commit + open, half of a late sumcheck round.  So: poll the completion signal (hipStreamQuery /
// hipEventQuery read it from memory) for up to ZIP_HIP_SPIN_US microseconds (default 4000; 0 = never), then block.
static long spin_budget_us() {
    static const long us = env_long("ZIP_HIP_SPIN_US", 4000, 0, LONG_MAX);
    return us;
}
// hipErrorNotReady may be left behind as the thread's "last error" by a poll: the launch checks must not find it --
// but a GENUINE pending error (a failed launch somebody checks later) must stay where it is.
static inline void clear_not_ready() {
    if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();
}
template <class Query>
static inline bool spin_until_done(Query query, hipError_t *result) {
    const long budget = spin_budget_us();
    if (budget <= 0) return false;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; it++) {
        const hipError_t e = query();
        if (e != hipErrorNotReady) { if (it) clear_not_ready(); *result = e; return true; }
        if ((it & 15u) == 15u &&
            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > budget) {
            clear_not_ready();
            return false;
        }
    }
}
static hipError_t stream_wait(hipStream_t s) {
    hipError_t e = hipSuccess;
    if (spin_until_done([s] { return hipStreamQuery(s); }, &e)) return e;
    return hipStreamSynchronize(s);
}
static hipError_t event_wait(hipEvent_t ev) {
    hipError_t e = hipSuccess;
    if (spin_until_done([ev] { return hipEventQuery(ev); }, &e)) return e;
    return hipEventSynchronize(ev);
}

// Device blocks of dead short-lived contexts (ctx->recycle), per device, exact-size lists.  A block enters
// only after its context synchronised every stream it had, so the next owner may use it at once.
struct RecycleBin {
    std::mutex mu;
    std::multimap<size_t, void *> blocks;
    size_t bytes = 0;
    unsigned char *bounce[2] = {nullptr, nullptr};  // one spare pair of pinned bounce buffers (hipHostMalloc is ~10 ms)
    size_t bounce_cap = 0;
};
constexpr int kMaxDevices = 16;
constexpr size_t kRecycleCapBytes = (size_t)4 << 30;
RecycleBin g_recycle[kMaxDevices];

void *recycle_take(int device, size_t bytes) {
    if (device < 0 || device >= kMaxDevices) return nullptr;
    RecycleBin &bin = g_recycle[device];
    std::lock_guard<std::mutex> g(bin.mu);
    auto it = bin.blocks.find(bytes);
    if (it == bin.blocks.end()) return nullptr;
    void *p = it->second;
    bin.blocks.erase(it);
    bin.bytes -= bytes;
    return p;
}
void recycle_give(int device, size_t bytes, void *p) {
    if (device >= 0 && device < kMaxDevices) {
        RecycleBin &bin = g_recycle[device];
        std::lock_guard<std::mutex> g(bin.mu);
        if (bin.bytes + bytes <= kRecycleCapBytes) {
            bin.blocks.emplace(bytes, p);
            bin.bytes += bytes;
            return;
        }
    }
    (void)hipFree(p);
}
void recycle_flush(int device) {
    if (device < 0 || device >= kMaxDevices) return;
    RecycleBin &bin = g_recycle[device];
    std::lock_guard<std::mutex> g(bin.mu);
    for (auto &kv : bin.blocks) (void)hipFree(kv.second);
    bin.blocks.clear();
    bin.bytes = 0;
    for (auto *&b : bin.bounce) {
        if (b) (void)hipHostFree(b);
        b = nullptr;
    }
    bin.bounce_cap = 0;
}

// 256-byte slots of host-mapped pinned memory for results a kernel hands straight to the host (a sumcheck round
// message is at most 160 bytes): one hipHostMalloc per device, ever.
constexpr uint32_t kSlabSlots = 256, kSlabSlotBytes = 256;
struct PinnedSlab {
    std::mutex mu;
    unsigned char *base = nullptr;
    bool used[kSlabSlots] = {};
};
PinnedSlab g_slab[kMaxDevices];
unsigned char *slab_take(int device) {
    if (device < 0 || device >= kMaxDevices) return nullptr;
    PinnedSlab &sl = g_slab[device];
    std::lock_guard<std::mutex> g(sl.mu);
    if (!sl.base && hipHostMalloc((void **)&sl.base, (size_t)kSlabSlots * kSlabSlotBytes, hipHostMallocCoherent) != hipSuccess) {
        sl.base = nullptr;
        return nullptr;
    }
    for (uint32_t i = 0; i < kSlabSlots; i++)
        if (!sl.used[i]) {
            sl.used[i] = true;
            return sl.base + (size_t)i * kSlabSlotBytes;
        }
    return nullptr;
}
void slab_give(int device, unsigned char *p) {
    if (!p || device < 0 || device >= kMaxDevices) return;
    PinnedSlab &sl = g_slab[device];
    std::lock_guard<std::mutex> g(sl.mu);
    sl.used[(p - sl.base) / kSlabSlotBytes] = false;
}

int32_t pool_alloc(zip_ctx *ctx, size_t bytes, void **out) {
    *out = nullptr;
    if (bytes == 0) bytes = 16;
    std::lock_guard<std::mutex> g(ctx->mu);
    auto it = ctx->free_blocks.find(bytes);
    if (it != ctx->free_blocks.end()) {
        *out = it->second;
        ctx->free_blocks.erase(it);
    } else if (ctx->recycle && (*out = recycle_take(ctx->device, bytes))) {
    } else {
        hipError_t e = hipMalloc(out, bytes);
        if (e != hipSuccess) {
            // release cached blocks and retry once
            for (auto &kv : ctx->free_blocks) (void)hipFree(kv.second);
            ctx->free_blocks.clear();
            recycle_flush(ctx->device);
            e = hipMalloc(out, bytes);
            if (e != hipSuccess)
                return fail(ctx, ZIP_ERR_ALLOC, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        }
    }
    ctx->live_blocks[*out] = bytes;
    return ZIP_OK;
}

void pool_release(zip_ctx *ctx, void *ptr) {
    if (!ptr) return;
    std::lock_guard<std::mutex> g(ctx->mu);
    auto it = ctx->live_blocks.find(ptr);
    if (it == ctx->live_blocks.end()) return;
    ctx->free_blocks.emplace(it->second, ptr);
    ctx->live_blocks.erase(it);
}

// RAII for temporaries taken from the pool.  Stream order makes reuse safe: every
// consumer of a block is enqueued on ctx->stream before the block can be handed out again.
struct Scratch {
    zip_ctx *ctx;
    void *ptr = nullptr;
    explicit Scratch(zip_ctx *c) : ctx(c) {}
    ~Scratch() { pool_release(ctx, ptr); }
    int32_t get(size_t bytes) { return pool_alloc(ctx, bytes, &ptr); }
    template <class T>
    T *as() { return static_cast<T *>(ptr); }
};

// Copies up to three small host arrays into ONE device block through the pinned staging
// buffer.  The staging buffer is reused by the next call, so every caller synchronises the
// stream before returning (they all do: host inputs must be consumed before we return).
struct SmallInputs {
    static constexpr int N = 7;
    const void *src[N] = {};
    size_t bytes[N] = {};
    size_t off[N] = {};
};
// own_stage / own_cap: a pinned buffer of the caller's instead of the ctx's (a job that returns before the copy has run)
int32_t stage_small(zip_ctx *ctx, SmallInputs &in, Scratch &dev, unsigned char **base, unsigned char *own_stage = nullptr,
                    size_t own_cap = 0) {
    size_t total = 0;
    for (int i = 0; i < SmallInputs::N; i++) {
        in.off[i] = total;
        total += (in.bytes[i] + 255) & ~(size_t)255;
    }
    if (total == 0) { *base = nullptr; return ZIP_OK; }
    unsigned char *stage = own_stage ? own_stage : ctx->stage_h;
    if (own_stage) {
        if (total > own_cap) return fail(ctx, ZIP_ERR_UNSUPPORTED, "small inputs (%zu bytes) exceed a job's staging block", total);
    } else if (total > ctx->stage_cap) {
        // larger than the block allocated with the ctx (which also holds the timeout flag and
        // stays where it is): a second pinned buffer, grown on demand
        if (total > ctx->stage_big_cap) {
            if (ctx->stage_big) (void)hipHostFree(ctx->stage_big);
            ctx->stage_big = nullptr;
            ctx->stage_big_cap = 0;
            hipError_t e = hipHostMalloc((void **)&ctx->stage_big, total, hipHostMallocDefault);
            if (e != hipSuccess) return fail(ctx, ZIP_ERR_ALLOC, "hipHostMalloc(%zu) failed: %s", total, hipGetErrorString(e));
            ctx->stage_big_cap = total;
        }
        stage = ctx->stage_big;
    }
    for (int i = 0; i < SmallInputs::N; i++)
        if (in.bytes[i]) memcpy(stage + in.off[i], in.src[i], in.bytes[i]);
    int32_t rc = dev.get(total);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dev.ptr, stage, total, hipMemcpyHostToDevice, ctx->stream));
    *base = dev.as<unsigned char>();
    return ZIP_OK;
}

// ------------------------------------------------------------------ measurement
hipEvent_t take_event(zip_ctx *ctx) {
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct LaunchTimer {
    zip_ctx *ctx;
    hipStream_t st;
    PendingEvent pe{};
    bool on;
    LaunchTimer(zip_ctx *c, const char *name, hipStream_t stream = nullptr)
        : ctx(c), st(stream ? stream : c->stream), on(c->profiling) {
        // (events between the kernels of one stream cost each dependent launch ~12 us: mode 2 only brackets the
        // commit / encode kernel, which has its stream to itself)
        if (on && c->profile_commit_only && strncmp(name, "raa_", 4) != 0) on = false;
        if (!on) return;
        pe.name = name;
        pe.start = take_event(ctx);
        pe.stop = take_event(ctx);
        (void)hipEventRecord(pe.start, st);
    }
    ~LaunchTimer() {
        if (!on) return;
        (void)hipEventRecord(pe.stop, st);
        ctx->pending.push_back(pe);
    }
};

hipEvent_t take_dep_event(zip_ctx *ctx) {
    if (!ctx->dep_event_pool.empty()) {
        hipEvent_t e = ctx->dep_event_pool.back();
        ctx->dep_event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    return e;
}

// ------------------------------------------------------------------ large host <-> device copies
// hipMemcpy to or from pageable memory the runtime has not seen before first PINS it (measured:
// a fresh 383 MiB destination costs ~100 ms, 3-4 GB/s; the same buffer reused runs at 54 GB/s).
// The reference's calling convention hands over fresh Vecs every time, so large transfers go through
// two library-owned pinned bounce buffers instead: PCIe copy of chunk i beside a multi-threaded
// memcpy of chunk i-1 between the bounce buffer and the caller's memory.
constexpr size_t kBounceBytes = (size_t)32 << 20;
constexpr size_t kBounceThreshold = (size_t)8 << 20;

int32_t ensure_bounce(zip_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->bounce_cap) return ZIP_OK;
    if (ctx->recycle && !ctx->bounce[0] && ctx->device >= 0 && ctx->device < kMaxDevices) {
        RecycleBin &bin = g_recycle[ctx->device];
        std::lock_guard<std::mutex> g(bin.mu);
        if (bin.bounce_cap >= bytes) {
            for (int i = 0; i < 2; i++) {
                ctx->bounce[i] = bin.bounce[i];
                bin.bounce[i] = nullptr;
            }
            ctx->bounce_cap = bin.bounce_cap;
            bin.bounce_cap = 0;
            return ZIP_OK;
        }
    }
    for (auto *&b : ctx->bounce) {
        if (b) (void)hipHostFree(b);
        b = nullptr;
    }
    ctx->bounce_cap = 0;
    for (auto *&b : ctx->bounce) {
        hipError_t e = hipHostMalloc((void **)&b, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return fail(ctx, ZIP_ERR_ALLOC, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    ctx->bounce_cap = bytes;
    return ZIP_OK;
}

// Hands the pinned bounce pair of a short-lived context back (to the recycle bin, or to the driver) once its
// uploads are done: several such contexts may be alive at once (the products of a sum-of-products sumcheck) and
// 64 MiB of pinned memory each is neither cheap to allocate nor to hold.
void bounce_release(zip_ctx *ctx) {
    if (!ctx->bounce[0]) return;
    if (ctx->recycle && ctx->bounce[1] && ctx->device >= 0 && ctx->device < kMaxDevices) {
        RecycleBin &bin = g_recycle[ctx->device];
        std::lock_guard<std::mutex> g(bin.mu);
        if (!bin.bounce_cap) {
            for (int i = 0; i < 2; i++) {
                bin.bounce[i] = ctx->bounce[i];
                ctx->bounce[i] = nullptr;
            }
            bin.bounce_cap = ctx->bounce_cap;
        }
    }
    for (auto *&b : ctx->bounce) {
        if (b) (void)hipHostFree(b);
        b = nullptr;
    }
    ctx->bounce_cap = 0;
}

void parallel_memcpy(void *dst, const void *src, size_t bytes) {
    if (bytes < ((size_t)4 << 20)) {
        memcpy(dst, src, bytes);
        return;
    }
    static const unsigned n_env = (unsigned)env_long("ZIP_HIP_COPY_THREADS", 0, 0, INT_MAX);
    unsigned n = std::thread::hardware_concurrency();
    n = n_env ? std::min(n_env, 64u) : n ? std::min(n, 8u) : 4u;
    const size_t per = (((bytes + n - 1) / n) + 4095) & ~(size_t)4095;  // n * per >= bytes (a truncating bytes / n lost a tail of < n bytes)
    std::vector<std::thread> th;
    for (unsigned t = 1; t < n; t++) {
        const size_t lo = (size_t)t * per;
        if (lo >= bytes) break;
        const size_t len = std::min(per, bytes - lo);
        th.emplace_back([=] { memcpy(static_cast<char *>(dst) + lo, static_cast<const char *>(src) + lo, len); });
    }
    memcpy(dst, src, std::min(per, bytes));
    for (auto &x : th) x.join();
}

// true when the whole host range was pinned with zip_host_register / hipHostRegister / hipHostMalloc: the DMA
// engines can then reach it directly and the bounce copy (which runs at ~33 GB/s, not PCIe's 55) is skipped
bool host_range_is_pinned(const void *p, size_t bytes) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // an unknown (pageable) pointer is reported as an error: clear it
        return false;
    }
    if (a.type != hipMemoryTypeHost) return false;
    hipPointerAttribute_t b{};
    if (hipPointerGetAttributes(&b, static_cast<const char *>(p) + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return b.type == hipMemoryTypeHost;
}

// dst_h (pageable) <- src_d, ordered after everything enqueued on `after` so far.  Synchronous.
int32_t copy_d2h_bounced(zip_ctx *ctx, void *dst_h, const void *src_d, size_t bytes, hipStream_t after) {
    if (bytes >= kBounceThreshold && host_range_is_pinned(dst_h, bytes)) {
        HIP_TRY(ctx, hipMemcpyAsync(dst_h, src_d, bytes, hipMemcpyDeviceToHost, after));
        HIP_TRY(ctx, stream_wait(after));
        return ZIP_OK;
    }
    if (bytes < kBounceThreshold) {
        HIP_TRY(ctx, hipMemcpyAsync(dst_h, src_d, bytes, hipMemcpyDeviceToHost, after));
        HIP_TRY(ctx, stream_wait(after));
        return ZIP_OK;
    }
    int32_t rc = ensure_bounce(ctx, kBounceBytes);
    if (rc) return rc;
    const size_t chunk = ctx->bounce_cap;
    const size_t n = (bytes + chunk - 1) / chunk;
    hipEvent_t ev[2] = {take_dep_event(ctx), take_dep_event(ctx)};
    auto issue = [&](size_t i) -> int32_t {
        const size_t off = i * chunk, len = std::min(chunk, bytes - off);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->bounce[i & 1], static_cast<const char *>(src_d) + off, len, hipMemcpyDeviceToHost, after));
        HIP_TRY(ctx, hipEventRecord(ev[i & 1], after));
        return ZIP_OK;
    };
    rc = issue(0);
    for (size_t i = 0; i < n && rc == ZIP_OK; i++) {
        if (i + 1 < n) rc = issue(i + 1);  // bounce[(i+1)&1] was drained in iteration i-1
        if (rc) break;
        if (event_wait(ev[i & 1]) != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "device-to-host copy failed"); break; }
        const size_t off = i * chunk, len = std::min(chunk, bytes - off);
        parallel_memcpy(static_cast<char *>(dst_h) + off, ctx->bounce[i & 1], len);
    }
    (void)stream_wait(after);
    ctx->dep_event_pool.push_back(ev[0]);
    ctx->dep_event_pool.push_back(ev[1]);
    return rc;
}

// dst_d <- src_h (pageable) on `st`.  Returns once the caller's buffer has been read completely
// (the last chunk may still be in flight from the bounce buffer; later work on `st` is ordered).
int32_t copy_h2d_bounced(zip_ctx *ctx, void *dst_d, const void *src_h, size_t bytes, hipStream_t st) {
    if (bytes >= ctx->h2d_bounce_threshold && host_range_is_pinned(src_h, bytes)) {
        HIP_TRY(ctx, hipMemcpyAsync(dst_d, src_h, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, stream_wait(st));  // same contract as below: the caller's buffer is free on return
        return ZIP_OK;
    }
    if (bytes < ctx->h2d_bounce_threshold) {
        HIP_TRY(ctx, hipMemcpyAsync(dst_d, src_h, bytes, hipMemcpyHostToDevice, st));
        return ZIP_OK;
    }
    int32_t rc = ensure_bounce(ctx, kBounceBytes);
    if (rc) return rc;
    const size_t chunk = ctx->bounce_cap;
    const size_t n = (bytes + chunk - 1) / chunk;
    hipEvent_t ev[2] = {take_dep_event(ctx), take_dep_event(ctx)};
    for (size_t i = 0; i < n; i++) {
        const size_t off = i * chunk, len = std::min(chunk, bytes - off);
        if (i >= 2 && event_wait(ev[i & 1]) != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "host-to-device copy failed"); break; }
        parallel_memcpy(ctx->bounce[i & 1], static_cast<const char *>(src_h) + off, len);
        hipError_t e = hipMemcpyAsync(static_cast<char *>(dst_d) + off, ctx->bounce[i & 1], len, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(ev[i & 1], st);
        if (e != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "host-to-device copy failed: %s", hipGetErrorString(e)); break; }
    }
    // the bounce buffers are reused by the next call: wait for the tail
    (void)event_wait(ev[0]);
    (void)event_wait(ev[1]);
    ctx->dep_event_pool.push_back(ev[0]);
    ctx->dep_event_pool.push_back(ev[1]);
    return rc;
}

// Orders `stream` after the whole commit that produces `c`.
int32_t wait_ready(zip_commitment *c, hipStream_t stream) {
    if (c->done) HIP_TRY(c->ctx, hipStreamWaitEvent(stream, c->done, 0));
    return ZIP_OK;
}

// ------------------------------------------------------------------ field setup
int cmp_limbs(const uint64_t *a, const uint64_t *b, uint32_t n) {
    for (uint32_t i = n; i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
void sub_limbs(uint64_t *a, const uint64_t *b, uint32_t n) {
    uint64_t borrow = 0;
    for (uint32_t i = 0; i < n; i++) {
        u128 d = (u128)a[i] - b[i] - borrow;
        a[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
}
void dbl_mod(uint64_t *x, const uint64_t *q, uint32_t n) {
    const uint64_t top = x[n - 1] >> 63;
    for (uint32_t i = n; i-- > 1;) x[i] = (x[i] << 1) | (x[i - 1] >> 63);
    x[0] <<= 1;
    if (top || cmp_limbs(x, q, n) >= 0) sub_limbs(x, q, n);
}

// FieldConfig::new (src/field/config.rs:174-214): R, R^2 mod q and -q^-1 mod 2^64.
int32_t make_field_uncached(zip_ctx *ctx, const zip_field *zf, HostField *f);
// FieldConfig::new for the field of this call; the last one is remembered per context (R and R^2 are 512 modular
// doublings of multi-limb integers: ~10 us on the host, in front of every launch of a proof's PCS step)
int32_t make_field(zip_ctx *ctx, const zip_field *zf, HostField *f) {
    if (!zf) return fail(ctx, ZIP_ERR_NULL, "field is NULL");
    if (ctx && ctx->field_cache_valid && ctx->field_cache_in.limbs == zf->limbs &&
        !memcmp(ctx->field_cache_in.modulus, zf->modulus, 8 * (size_t)zf->limbs)) {
        *f = ctx->field_cache_out;
        return ZIP_OK;
    }
    int32_t rc = make_field_uncached(ctx, zf, f);
    if (!rc && ctx) {
        ctx->field_cache_in = *zf;
        ctx->field_cache_out = *f;
        ctx->field_cache_valid = true;
    }
    return rc;
}
int32_t make_field_uncached(zip_ctx *ctx, const zip_field *zf, HostField *f) {
    if (!zf) return fail(ctx, ZIP_ERR_NULL, "field is NULL");
    if (zf->limbs < 2 || zf->limbs > 4)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "field limbs %u not in {2,3,4}", zf->limbs);
    if (!(zf->modulus[0] & 1)) return fail(ctx, ZIP_ERR_INVALID_PARAM, "modulus must be odd");
    const uint32_t n = f->fl = zf->limbs;
    bool gt1 = zf->modulus[0] > 1;
    for (uint32_t i = 1; i < n; i++) gt1 |= zf->modulus[i] != 0;
    if (!gt1) return fail(ctx, ZIP_ERR_INVALID_PARAM, "modulus must be > 1");
    memcpy(f->modulus, zf->modulus, 8 * n);
    uint64_t inv = 1;
    for (int i = 0; i < 63; i++) {
        inv *= inv;
        inv *= f->modulus[0];
    }
    f->inv = (uint64_t)0 - inv;
    uint64_t x[8] = {1};
    for (uint32_t i = 0; i < 64 * n; i++) dbl_mod(x, f->modulus, n);
    memcpy(f->r, x, 8 * n);
    for (uint32_t i = 0; i < 64 * n; i++) dbl_mod(x, f->modulus, n);
    memcpy(f->r2, x, 8 * n);
    // A modulus with its top bit set is a negative Int<FL> inside the reference's `%=`
    // (src/field.rs:550-557, F::I = Int<N> at src/field.rs:280); observable for 64-bit
    // witnesses only when 2^(64 FL) - q < 2^64.
    f->quirk_mod = 0;
    if (f->modulus[n - 1] >> 63) {
        uint64_t m[8] = {0};
        sub_limbs(m, f->modulus, n);  // 2^(64n) - q
        bool small = true;
        for (uint32_t i = 1; i < n; i++) small &= (m[i] == 0);
        if (small) f->quirk_mod = m[0];
    }
    return ZIP_OK;
}

template <int FL>
FieldDev<FL> to_dev(const HostField &h) {
    FieldDev<FL> d;
    for (int i = 0; i < FL; i++) {
        d.modulus[i] = h.modulus[i];
        d.r2[i] = h.r2[i];
    }
    d.inv = h.inv;
    return d;
}

// fn(std::integral_constant<int, FL>) for a field of fl limbs (2, 3 or 4: make_field admits no other)
template <class Fn>
auto with_fl(uint32_t fl, Fn &&fn) {
    switch (fl) {
        case 2: return fn(std::integral_constant<int, 2>{});
        case 3: return fn(std::integral_constant<int, 3>{});
        default: return fn(std::integral_constant<int, 4>{});
    }
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the function ON ONE DEVICE: remembered per
// (function, device), under a lock -- contexts of different devices (and threads) share these launch helpers.
int32_t ensure_dynamic_lds(zip_ctx *ctx, const void *kern, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> granted;
    std::lock_guard<std::mutex> g(mu);
    size_t &have = granted[std::make_pair(kern, ctx->device)];
    if (bytes > have) {
        HIP_TRY(ctx, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        have = bytes;
    }
    return ZIP_OK;
}

// ------------------------------------------------------------------ commit dispatch
// Persistent launch: as many workgroups as stay resident together (at most one per row).
template <int E, bool HASH, int MODE = kStoreAll, bool CODES = false>
int32_t launch_commit(zip_ctx *ctx, const CommitArgs &a, uint32_t threads, uint32_t grid, hipStream_t st) {
    // wave totals + E planes of (threads + 32/E) slots of 12 bytes + the witness row (+ the opening tables)
    size_t lds = 512 + (size_t)E * (threads + 32 / E) * 12 + (size_t)a.row_len * 8 + 4 * kFinisherFlagWords;
    auto kern = raa_commit_kernel<E, HASH, MODE, CODES>;
    if (int32_t rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), lds)) return rc;
    LaunchTimer t(ctx, HASH ? "raa_commit_kernel" : "raa_encode_kernel", st);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

// raa_commit16_kernel (t2 compacted into LDS, T threads x 16 entries): cw = 16384 with T = 1024
template <bool HASH, int MODE = kStoreAll>
int32_t launch_commit16(zip_ctx *ctx, const CommitArgs &a, uint32_t grid, hipStream_t st) {
    constexpr uint32_t T = 1024;
    auto kern = raa_commit16_kernel<T, HASH, MODE>;
    if (int32_t rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), c16_lds_bytes(T))) return rc;
    LaunchTimer t(ctx, HASH ? "raa_commit_kernel" : "raa_encode_kernel", st);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(T), c16_lds_bytes(T), st, a);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

// raa_commit_slab_kernel (first accumulation through a global slab per workgroup): cw = 32768 / 65536, 1024 threads x
// cw / 1024 entries
template <bool HASH>
int32_t launch_commit_slab(zip_ctx *ctx, const CommitArgs &a, uint32_t grid, hipStream_t st) {
    auto kern = a.cw == 65536 ? raa_commit_slab_kernel<64, HASH> : raa_commit_slab_kernel<32, HASH>;
    if (int32_t rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), cslab_lds_bytes())) return rc;
    LaunchTimer t(ctx, HASH ? "raa_commit_kernel" : "raa_encode_kernel", st);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kSlabThreads), cslab_lds_bytes(), st, a);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

struct CommitGeom {
    uint32_t e, threads;
    size_t lds;
};
CommitGeom commit_geom(uint32_t cw, uint32_t row_len) {
    CommitGeom g{};
    if (cw >= 32768) { g.e = cw / kSlabThreads; g.threads = kSlabThreads; g.lds = cslab_lds_bytes(); return g; }
    if (cw == 16384) { g.e = 16; g.threads = 1024; g.lds = c16_lds_bytes(1024); return g; }
    // (cw = 8192 as two 512-thread workgroups of the 16-entry kernel per CU was measured and removed: 1.29 against
    // 1.35 ms alone at 2^24, but 1.99-2.17 against 1.76-1.79 ms per step -- it leaves the gathers 7 KB of LDS,
    // EXPERIMENTS.md.)
    if (cw >= 512) { g.e = 8; g.threads = cw / 8; }
    else if (cw == 256) { g.e = 4; g.threads = 64; }
    else if (cw == 128) { g.e = 2; g.threads = 64; }
    else { g.e = 1; g.threads = 64; }  // cw <= 64: one entry per lane
    g.lds = 512 + (size_t)g.e * (g.threads + 32 / g.e) * 12 + (size_t)row_len * 8 + 4 * kFinisherFlagWords;
    return g;
}
// resident workgroups per CU of the commit kernel (threads and LDS)
uint32_t commit_wgs_per_cu(const CommitGeom &g) {
    if (g.e > 16) return 1;  // the slab kernel: 1024 threads at up to 128 VGPRs fill a CU's register files
    uint32_t by_threads = 2048 / g.threads, by_lds = (uint32_t)((160u * 1024u) / g.lds);
    uint32_t k = by_threads < by_lds ? by_threads : by_lds;
    if (k > 8) k = 8;
    return k ? k : 1;
}

// geometries whose commit kernel has a hint-masked variant (smaller ones store everything: the hint is dropped)
// (and above cw 16384 neither: the slab kernel stores everything, and kHintBytes and the u16 rank tables are sized for
// cw <= 16384 -- a hinted or packed commit there is not built)
bool commit_supports_hint(uint32_t cw) { return cw >= 512 && cw <= 16384; }
// one pinned / device block per hinted commit: the bitmaps (<= 5.6 KB for cw <= 16384) at offset 0, the
// column -> openings tables of zip_commit_open (first[cw] | next[n_cols], u16) at kHintTables
// (packed openings: the rank table at kHintTables -- up to 8 bytes for each of 1024 threads --, the ranks of the hinted
// openings at kPackedRanksAt)
constexpr uint32_t kRingSlots = 64, kRingChunks = 16, kRingStride = 16;  // zip_ctx::ring_d
constexpr size_t kHintTables = 8192, kPackedRanksAt = kHintTables + 8192, kHintBytes = kPackedRanksAt + 8 * (8192 / 32) + 4 * 4096 + 64;
// ---- opening hints and packed openings (CommitArgs.need / .pk) -------------------------------------------------
// Everything a hinted commit derives from its column list, kept per ctx until the list changes (in the prover flow it
// never does: a fresh PcsTranscript squeezes the same columns for every proof, zinc/prover.rs:316).
//   bm         the four bitmaps V | N0 (cw bits each) | N1 (cw / 2) | N2 (cw / 4): entries opened, level-0..2 nodes
//              that are some opening's sibling
//   packed     the commit kernel of this geometry can store those members densely (CommitArgs.pk); then
//   pos[s][i]  = the place of member i in section s of a row's packed block, and rank_tab = CommitArgs.pk_tab.
// The place of a member is its turn in the enumeration  wave -> output phase -> store site -> lane class -> lane
// of the kernel's lanes (StridedLeaves: entry of step e = e * sT + stid(lane); level-1 node of group g at lane
// parity p = ((2g + p) sT + stid) >> 1; level-2 node of group g at lane mod 4 = c = ((4g + c) sT + stid) >> 2): the
// kernel recovers it as a per-wave base (rank_tab) + the number of storing lanes of the class below it.
// The 8-entries-per-thread kernel keeps natural ownership (OwnLeaves8: lane t owns entries 8t.., level-1 nodes 4t..,
// level-2 nodes 2t..): its enumeration is plain index order, and rank_tab holds per LANE the number of members of each
// section below the lane's first -- the kernel adds the lane's own members below the one it stores.
static bool packed_enabled() {
    return env_long("ZIP_HIP_PACKED", 1, 0, 1) != 0;  // (read per call: the tests flip it)
}
// the four sections of a row's packed block, each a whole number of 128-byte lines, from their member counts
static void packed_layout(HintPlan &P, const uint32_t (&cnt)[4]) {
    uint32_t at = (cnt[0] * 16u + 127u) & ~127u;
    P.L.off[0] = at;
    at = (at + cnt[1] * 32u + 127u) & ~127u;
    P.L.off[1] = at;
    at = (at + cnt[2] * 32u + 127u) & ~127u;
    P.L.off[2] = at;
    at = (at + cnt[3] * 32u + 127u) & ~127u;
    P.L.stride = at;
}
struct HintSections {  // the four bitmaps of a plan and their sizes in bits
    const uint32_t *sec[4];
    uint32_t bits[4];
    explicit HintSections(const HintPlan &P) {
        const uint32_t cw = P.cw, wv = (cw + 31) / 32, w1 = (cw / 2 + 31) / 32;
        const uint32_t *b = P.bm.data();
        sec[0] = b, sec[1] = b + wv, sec[2] = b + 2 * wv, sec[3] = b + 2 * wv + w1;
        bits[0] = cw, bits[1] = cw, bits[2] = cw / 2, bits[3] = cw / 4;
    }
    uint32_t member(int k, uint32_t i) const { return (sec[k][i >> 5] >> (i & 31u)) & 1u; }
};
// raa_commit_kernel<8, ..., kStorePacked> (natural ownership): index order; rank_tab = [threads][2] per-lane bases
static void plan_packed_own8(HintPlan &P) {
    const HintSections S(P);
    for (int k = 0; k < 4; k++) P.pos[k].assign(S.bits[k], 0xFFFF);
    uint32_t cnt[4] = {0, 0, 0, 0};
    P.rank_tab.assign((size_t)P.threads * 2, 0);
    for (uint32_t t = 0; t < P.threads; t++) {
        P.rank_tab[2 * t] = cnt[0] | (cnt[1] << 16);
        P.rank_tab[2 * t + 1] = cnt[2] | (cnt[3] << 16);
        for (int k = 0; k < 4; k++) {
            const uint32_t per = S.bits[k] / P.threads;  // 8, 8, 4, 2 members of lane t at most
            for (uint32_t i = t * per; i < (t + 1) * per; i++)
                if (S.member(k, i)) P.pos[k][i] = (uint16_t)cnt[k]++;
        }
    }
    packed_layout(P, cnt);
}
// raa_commit16_kernel<..., kStorePacked> (strided ownership inside 8-lane groups, two output phases): the enumeration
// above; rank_tab = [waves][2][16] words of per-wave bases
static void plan_packed_strided16(HintPlan &P) {
    const HintSections S(P);
    const uint32_t waves = P.threads / 64, phases = 2, sT = 16;
    for (int k = 0; k < 4; k++) P.pos[k].assign(S.bits[k], 0xFFFF);
    P.rank_tab.assign((size_t)waves * phases * 16, 0);
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t w = 0; w < waves; w++)
        for (uint32_t q = 0; q < phases; q++) {
            uint16_t base[32];
            auto stid = [&](uint32_t l) {
                const uint32_t tid = 64 * w + l;
                return (tid & ~7u) * 16u + q * 8u + (tid & 7u);
            };
            auto site = [&](int k, int slot, uint32_t step, uint32_t shift, uint32_t cls, uint32_t ncls) {
                base[slot] = (uint16_t)cnt[k];
                for (uint32_t l = cls; l < 64; l += ncls) {
                    const uint32_t i = (step * sT + stid(l)) >> shift;
                    if (S.member(k, i)) P.pos[k][i] = (uint16_t)cnt[k]++;
                }
            };
            for (uint32_t e = 0; e < 8; e++) site(0, (int)e, e, 0, 0, 1);
            for (uint32_t e = 0; e < 8; e++) site(1, (int)(8 + e), e, 0, 0, 1);
            for (uint32_t g = 0; g < 4; g++)
                for (uint32_t par = 0; par < 2; par++) site(2, (int)(16 + 2 * g + par), 2 * g + par, 1, par, 2);
            for (uint32_t g = 0; g < 2; g++)
                for (uint32_t c4 = 0; c4 < 4; c4++) site(3, (int)(24 + 4 * g + c4), 4 * g + c4, 2, c4, 4);
            uint32_t *tab = P.rank_tab.data() + ((size_t)w * phases + q) * 16;
            for (uint32_t k = 0; k < 16; k++) tab[k] = (uint32_t)base[2 * k] | ((uint32_t)base[2 * k + 1] << 16);
        }
    packed_layout(P, cnt);
}
static void plan_packed(HintPlan &P) {
    if (P.e == 8) plan_packed_own8(P);
    else plan_packed_strided16(P);
}
// zip_commit_open stores the low part of the openings packed where the commit kernel has the variant (whole waves of
// 8 or 16 entries per thread, depth >= 3); the packed rows take the place of the 16-byte row entries (commit_impl sizes
// the buffer for whichever is larger: at cw <= 4096 a row's packed block exceeds its compact entries)
static std::shared_ptr<HintPlan> get_hint_plan(zip_ctx *ctx, const uint32_t *cols, uint32_t n_cols, bool want_packed) {
    const uint32_t cw = ctx->p.codeword_len;
    const CommitGeom g = commit_geom(cw, ctx->p.row_len);
    if (ctx->hint_plan) {
        const HintPlan &h = *ctx->hint_plan;
        if (h.cw == cw && h.e == g.e && h.threads == g.threads && h.want_packed == want_packed && h.cols.size() == n_cols &&
            (n_cols == 0 || !memcmp(h.cols.data(), cols, (size_t)n_cols * 4)))
            return ctx->hint_plan;
    }
    auto P = std::make_shared<HintPlan>();
    P->cw = cw;
    P->e = g.e;
    P->threads = g.threads;
    P->want_packed = want_packed;
    P->cols.assign(cols, cols + n_cols);
    const uint32_t wv = (cw + 31) / 32, w1 = (cw / 2 + 31) / 32, w2 = (cw / 4 + 31) / 32;
    P->bm.assign(2 * (size_t)wv + w1 + w2, 0);
    uint32_t *nv = P->bm.data(), *n0 = nv + wv, *n1 = n0 + wv, *n2 = n1 + w1;
    for (uint32_t i = 0; i < n_cols; i++) {
        const uint32_t col = cols[i];
        nv[col >> 5] |= 1u << (col & 31);
        const uint32_t s0 = col ^ 1u, s1 = (col >> 1) ^ 1u, s2 = (col >> 2) ^ 1u;
        n0[s0 >> 5] |= 1u << (s0 & 31);
        n1[s1 >> 5] |= 1u << (s1 & 31);
        n2[s2 >> 5] |= 1u << (s2 & 31);
    }
    if (want_packed && n_cols && (g.e == 8 || g.e == 16) && cw >= 512 && g.threads % 64 == 0 && cw == g.e * g.threads &&
        ctx->depth >= 3) {
        plan_packed(*P);
        P->own_ranks.resize((size_t)n_cols * 4);
        P->packed = P->L.stride > 0 && P->rank_tab.size() * 4 <= kPackedRanksAt - kHintTables &&
                    kPackedRanksAt + P->own_ranks.size() * 2 <= kHintBytes && P->ranks(cols, n_cols, P->own_ranks.data());
    }
    // the tables go to the device here, once, not with every commit
    std::vector<unsigned char> img(kHintBytes, 0);
    memcpy(img.data(), P->bm.data(), P->bm.size() * 4);
    size_t used = P->bm.size() * 4;
    if (P->packed) {
        memcpy(img.data() + kHintTables, P->rank_tab.data(), P->rank_tab.size() * 4);
        memcpy(img.data() + kPackedRanksAt, P->own_ranks.data(), P->own_ranks.size() * 2);
        used = kPackedRanksAt + P->own_ranks.size() * 2;
    }
    void *blk = nullptr;
    if (used <= kHintBytes && pool_alloc(ctx, kHintBytes, &blk) == ZIP_OK) {
        if (hipMemcpy(blk, img.data(), used, hipMemcpyHostToDevice) == hipSuccess) {
            P->dev = static_cast<unsigned char *>(blk);
            std::shared_ptr<bool> alive = ctx->alive;  // (a handle that outlives its ctx must not touch the ctx's pool)
            P->release = [ctx, alive](unsigned char *p) { if (*alive) pool_release(ctx, p); };
        } else {
            pool_release(ctx, blk);
            (void)hipGetLastError();
        }
    }
    ctx->hint_plan = P;
    return P;
}

template <bool HASH>
int32_t dispatch_commit(zip_ctx *ctx, CommitArgs a, uint32_t grid, hipStream_t st) {
    const CommitGeom g = commit_geom(a.cw, a.row_len);
    a.nact = a.cw / g.e < g.threads ? a.cw / g.e : g.threads;
    if (HASH && a.need) {  // opening hint: only the two big geometries have a masked variant (commit_supports_hint)
        if (g.e == 8 && a.pk) return launch_commit<8, HASH, HASH ? kStorePacked : kStoreAll>(ctx, a, g.threads, grid, st);
        if (g.e == 16 && a.pk) return launch_commit16<HASH, HASH ? kStorePacked : kStoreAll>(ctx, a, grid, st);
        a.pk = nullptr;
        if (g.e == 16) return launch_commit16<HASH, HASH ? kStoreHinted : kStoreAll>(ctx, a, grid, st);
        if (g.e == 8) return launch_commit<8, HASH, HASH ? kStoreHinted : kStoreAll>(ctx, a, g.threads, grid, st);
        a.need = nullptr;
    }
    a.pk = nullptr;
    switch (g.e) {
        case 64:
        case 32: return launch_commit_slab<HASH>(ctx, a, grid, st);
        case 16: return launch_commit16<HASH>(ctx, a, grid, st);
        case 8: return launch_commit<8, HASH>(ctx, a, g.threads, grid, st);
        case 4: return launch_commit<4, HASH>(ctx, a, g.threads, grid, st);
        case 2: return launch_commit<2, HASH>(ctx, a, g.threads, grid, st);
        default: return launch_commit<1, HASH>(ctx, a, g.threads, grid, st);
    }
}

// zip_batch_commit_codes: a.perm1 / a.perm2 hold one slice per member of 2^a.log_member_rows rows.  Built for the
// geometries of raa_commit_kernel (cw <= 8192), stored in full and hashed.
constexpr uint32_t kMaxCodesCodeword = 8192;
int32_t dispatch_commit_codes(zip_ctx *ctx, CommitArgs a, uint32_t grid, hipStream_t st) {
    const CommitGeom g = commit_geom(a.cw, a.row_len);
    a.nact = a.cw / g.e < g.threads ? a.cw / g.e : g.threads;
    a.pk = nullptr;
    a.need = nullptr;
    switch (g.e) {
        case 8: return launch_commit<8, true, kStoreAll, true>(ctx, a, g.threads, grid, st);
        case 4: return launch_commit<4, true, kStoreAll, true>(ctx, a, g.threads, grid, st);
        case 2: return launch_commit<2, true, kStoreAll, true>(ctx, a, g.threads, grid, st);
        case 1: return launch_commit<1, true, kStoreAll, true>(ctx, a, g.threads, grid, st);
        default: return fail(ctx, ZIP_ERR_UNSUPPORTED, "a code per member is not built for codeword %u", a.cw);
    }
}

template <int NL>
int32_t launch_upper(zip_ctx *ctx, hipStream_t st, uint32_t *layers, uint32_t *roots, uint32_t trees, uint32_t cw,
                     uint32_t level_in, uint32_t depth) {
    const uint64_t total = (uint64_t)trees * ((cw >> level_in) >> NL);
    const uint32_t threads = 256;
    const uint32_t blocks = (uint32_t)((total + threads - 1) / threads);
    LaunchTimer t(ctx, "merkle_upper_kernel", st);
    hipLaunchKernelGGL(merkle_upper_kernel<NL>, dim3(blocks), dim3(threads), 0, st, layers, roots, trees, cw,
                       level_in, depth);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

int32_t merkle_upper_levels(zip_ctx *ctx, hipStream_t st, uint32_t *layers, uint32_t *roots, uint32_t trees,
                            uint32_t cw, uint32_t level, uint32_t depth) {
    if (depth == 0) {
        LaunchTimer t(ctx, "copy_roots_depth0_kernel", st);
        hipLaunchKernelGGL(copy_roots_depth0_kernel, dim3((trees + 255) / 256), dim3(256), 0, st, layers, roots,
                           trees, cw);
        HIP_TRY(ctx, hipGetLastError());
        return ZIP_OK;
    }
    while (level < depth) {
        const uint32_t rem = depth - level;
        int32_t rc;
        if (rem >= 4) {
            rc = launch_upper<4>(ctx, st, layers, roots, trees, cw, level, depth);
            level += 4;
        } else if (rem == 3) {
            rc = launch_upper<3>(ctx, st, layers, roots, trees, cw, level, depth);
            level += 3;
        } else if (rem == 2) {
            rc = launch_upper<2>(ctx, st, layers, roots, trees, cw, level, depth);
            level += 2;
        } else {
            rc = launch_upper<1>(ctx, st, layers, roots, trees, cw, level, depth);
            level += 1;
        }
        if (rc) return rc;
    }
    return ZIP_OK;
}

// Brings a witness shard onto the device if it is host memory.
int32_t stage_evals(zip_ctx *ctx, const int64_t *evals, zip_mem_kind kind, size_t n, Scratch &tmp,
                    const int64_t **dev) {
    if (!evals) return fail(ctx, ZIP_ERR_NULL, "evals is NULL");
    if (kind == ZIP_MEM_DEVICE) {
        *dev = evals;
        return ZIP_OK;
    }
    int32_t rc = tmp.get(n * 8);
    if (rc) return rc;
    if ((rc = copy_h2d_bounced(ctx, tmp.ptr, evals, n * 8, ctx->stream))) return rc;
    *dev = tmp.as<int64_t>();
    return ZIP_OK;
}

// ------------------------------------------------------------------ open pieces
struct CombineOut {
    uint64_t *uprime = nullptr;     // device
    uint64_t *row_limbs = nullptr;  // device
    uint8_t *row_be = nullptr;      // device
};

// The per-chunk partial sums of one combination: a caller that runs the two phases apart keeps them here between
// the calls.  Like every Scratch, its consumers are all enqueued on ctx->stream.
struct CombineScratch {
    Scratch pint, pa, pb;
    explicit CombineScratch(zip_ctx *c) : pint(c), pa(c), pb(c) {}
};

// Row chunks of the combination passes: enough workgroups to fill the chip, but few enough that the (latency-bound)
// fold of the partials in combine_finalize_kernel stays short -- 128 chunks at 2^20 cost 0.32 ms there
struct CombineChunks {
    uint32_t bx, chunks, rpc;
};
CombineChunks combine_chunks(const zip_ctx *ctx) {
    const uint32_t R = ctx->rows_local, C = ctx->p.row_len;
    const uint32_t bx = (C + 255) / 256;
    uint32_t chunks = 512 / bx;
    if (chunks > 32) chunks = 32;
    if (chunks < 1) chunks = 1;
    if (chunks > R) chunks = R;
    const uint32_t rpc = (R + chunks - 1) / chunks;
    chunks = (R + rpc - 1) / rpc;
    return {bx, chunks, rpc};
}

// coeffs_d / q0_d: DEVICE pointers (already staged)
template <int FL>
int32_t run_combine_fl(zip_ctx *ctx, const int64_t *evals_d, const int64_t *coeffs_dv,
                       const uint64_t *q0_dv, const HostField *hf, bool do_int, bool do_field, const CombineOut &out,
                       CombineScratch *ext, int phase) {
    // phase 0: both kernels; 1: only the pass over the witness (partial sums into `ext`); 2: only the fold of the
    // partial sums `ext` already holds.  zip_open runs them at the two ends of its pipeline.
    const uint32_t R = ctx->rows_local, C = ctx->p.row_len;
    const CombineChunks g = combine_chunks(ctx);
    const uint32_t bx = g.bx, chunks = g.chunks, rpc = g.rpc;

    const hipStream_t st = ctx->stream;
    CombineScratch own(ctx);
    CombineScratch &cs = ext ? *ext : own;
    Scratch &pint = cs.pint, &pa = cs.pa, &pb = cs.pb;
    int32_t rc;
    CombineArgs a{};
    a.evals = evals_d;
    a.num_rows = R;
    a.row_len = C;
    a.rows_per_chunk = rpc;
    a.prio = 1;
    a.quirk_mod = hf ? hf->quirk_mod : 0;
    if (do_int) {
        if (phase != 2 && (rc = pint.get((size_t)chunks * C * 3 * 8))) return rc;
        a.coeffs = coeffs_dv;
        a.part_int = pint.as<uint64_t>();
    }
    if (do_field) {
        if (phase != 2 && (rc = pa.get((size_t)chunks * C * (FL + 2) * 8))) return rc;
        a.q0 = q0_dv;
        a.part_a = pa.as<uint64_t>();
    }
    // the column-independent sums of every chunk (combine_rows_kernel: part_k)
    if (phase != 2 && (rc = pb.get((size_t)chunks * (FL + 3) * 8))) return rc;
    a.part_k = pb.as<uint64_t>();
    if (phase != 2) {
        LaunchTimer t(ctx, "combine_rows_kernel", st);
        const dim3 grid(bx, chunks), block(256);
        if (a.quirk_mod && do_field) {  // (rare moduli: the instance that carries the 64-bit division)
            if (do_int)
                hipLaunchKernelGGL((combine_rows_kernel<FL, true, true, true>), grid, block, 0, st, a);
            else
                hipLaunchKernelGGL((combine_rows_kernel<FL, false, true, true>), grid, block, 0, st, a);
        } else if (do_int && do_field)
            hipLaunchKernelGGL((combine_rows_kernel<FL, true, true, false>), grid, block, 0, st, a);
        else if (do_int)
            hipLaunchKernelGGL((combine_rows_kernel<FL, true, false, false>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((combine_rows_kernel<FL, false, true, false>), grid, block, 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    FinalizeArgs fa{};
    fa.part_int = a.part_int;
    fa.part_a = a.part_a;
    fa.part_k = a.part_k;
    fa.num_rows = R;
    fa.chunks = chunks;
    fa.row_len = C;
    fa.m_limbs = ctx->p.m_limbs;
    fa.prio = a.prio;
    fa.uprime = out.uprime;
    fa.row_limbs = out.row_limbs;
    fa.row_be = out.row_be;
    FieldDev<FL> fd{};
    if (hf) fd = to_dev<FL>(*hf);
    if (phase != 1) {
        LaunchTimer t(ctx, "combine_finalize_kernel", st);
        const dim3 grid((C + kFinalizeCols - 1) / kFinalizeCols), block(kFinalizeCols * kFinalizeGroups);
        if (do_int && do_field)
            hipLaunchKernelGGL((combine_finalize_kernel<FL, true, true>), grid, block, 0, st, fa, fd);
        else if (do_int)
            hipLaunchKernelGGL((combine_finalize_kernel<FL, true, false>), grid, block, 0, st, fa, fd);
        else
            hipLaunchKernelGGL((combine_finalize_kernel<FL, false, true>), grid, block, 0, st, fa, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    return ZIP_OK;
}

int32_t run_combine(zip_ctx *ctx, const int64_t *evals_d, const int64_t *coeffs_dv, const uint64_t *q0_dv,
                    const HostField *hf, bool do_int, bool do_field, const CombineOut &out,
                    CombineScratch *ext = nullptr, int phase = 0) {
    return with_fl(hf ? hf->fl : 4, [&](auto FL) {
        return run_combine_fl<decltype(FL)::value>(ctx, evals_d, coeffs_dv, q0_dv, hf, do_int, do_field, out, ext, phase);
    });
}

// ---- proximity tests beyond the first (zip_ctx_set_proximity_tests) ----
// What the single-context paths make of the ctx's count: a one-row matrix has no test at all, whatever the spec says
// (open_z.rs:100, verify_z.rs:66).
uint32_t proximity_tests(const zip_ctx *ctx) { return ctx->p.num_rows > 1 ? ctx->n_tests : 1; }
// bytes of u'_0 .. u'_{T-1} at the head of a proof stream (commit.rs:726)
size_t uprime_bytes(const zip_ctx *ctx) {
    return ctx->p.num_rows > 1 ? (size_t)proximity_tests(ctx) * ctx->p.row_len * ctx->p.m_limbs * 8 : 0;
}
// The paths that stay one-test paths (batches, row shards, several GPUs)
int32_t refuse_extra_tests(zip_ctx *ctx, const char *what) {
    if (ctx->n_tests > 1)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "%s serves one proximity test; the ctx is set to %u (use zip_open / zip_verify)", what,
                    ctx->n_tests);
    return ZIP_OK;
}

// u'_1 .. u'_{nt}: ONE pass over the witness for all of them (combine_rows_extra_kernel), then per test the integer fold
// that test 0 takes too, straight to the test's place in the stream.  Enqueued on ctx->stream behind test 0.
// coeffs_dv: [nt][rows] (device), uprime: [nt][row_len][m_limbs] (device).
constexpr int kExtraFoldFL = 4;  // the fold instance (its field half is compiled out; FL only sets the part_k stride)
int32_t run_combine_extra(zip_ctx *ctx, const int64_t *evals_d, const int64_t *coeffs_dv, uint32_t nt, uint64_t *uprime) {
    if (nt == 0) return ZIP_OK;
    if (nt > 7) return fail(ctx, ZIP_ERR_UNSUPPORTED, "%u proximity tests beside the first (at most 7)", nt);
    const uint32_t R = ctx->rows_local, C = ctx->p.row_len, M = ctx->p.m_limbs;
    const CombineChunks g = combine_chunks(ctx);
    const hipStream_t st = ctx->stream;
    Scratch pint(ctx), pk(ctx);
    int32_t rc;
    if ((rc = pint.get((size_t)nt * g.chunks * C * 3 * 8))) return rc;
    if ((rc = pk.get((size_t)nt * g.chunks * (kExtraFoldFL + 3) * 8))) return rc;
    CombineExtraArgs a{};
    a.evals = evals_d;
    a.coeffs = coeffs_dv;
    a.num_rows = R;
    a.row_len = C;
    a.rows_per_chunk = g.rpc;
    a.chunks = g.chunks;
    a.prio = 1;
    a.k_stride = kExtraFoldFL + 3;
    a.part_int = pint.as<uint64_t>();
    a.part_k = pk.as<uint64_t>();
    {
        LaunchTimer t(ctx, "combine_rows_extra_kernel", st);
        const dim3 grid(g.bx, g.chunks), block(256);
        switch (nt) {
            case 1: hipLaunchKernelGGL(combine_rows_extra_kernel<1>, grid, block, 0, st, a); break;
            case 2: hipLaunchKernelGGL(combine_rows_extra_kernel<2>, grid, block, 0, st, a); break;
            case 3: hipLaunchKernelGGL(combine_rows_extra_kernel<3>, grid, block, 0, st, a); break;
            case 4: hipLaunchKernelGGL(combine_rows_extra_kernel<4>, grid, block, 0, st, a); break;
            case 5: hipLaunchKernelGGL(combine_rows_extra_kernel<5>, grid, block, 0, st, a); break;
            case 6: hipLaunchKernelGGL(combine_rows_extra_kernel<6>, grid, block, 0, st, a); break;
            default: hipLaunchKernelGGL(combine_rows_extra_kernel<7>, grid, block, 0, st, a); break;
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    const FieldDev<kExtraFoldFL> unused{};
    for (uint32_t t = 0; t < nt; t++) {
        FinalizeArgs fa{};
        fa.part_int = a.part_int + (size_t)t * g.chunks * C * 3;
        fa.part_k = a.part_k + (size_t)t * g.chunks * a.k_stride;
        fa.num_rows = R;
        fa.chunks = g.chunks;
        fa.row_len = C;
        fa.m_limbs = M;
        fa.prio = a.prio;
        fa.uprime = uprime + (size_t)t * C * M;
        LaunchTimer tm(ctx, "combine_finalize_kernel", st);
        const dim3 grid((C + kFinalizeCols - 1) / kFinalizeCols), block(kFinalizeCols * kFinalizeGroups);
        hipLaunchKernelGGL((combine_finalize_kernel<kExtraFoldFL, true, false>), grid, block, 0, st, fa, unused);
        HIP_TRY(ctx, hipGetLastError());
    }
    return ZIP_OK;
}

int32_t check_cols(zip_ctx *ctx, const uint32_t *cols_h, uint32_t n_cols) {
    for (uint32_t i = 0; i < n_cols; i++)
        if (cols_h[i] >= ctx->p.codeword_len)
            return fail(ctx, ZIP_ERR_INVALID_PARAM, "column index %u out of range (codeword_len %u)", cols_h[i],
                        ctx->p.codeword_len);
    return ZIP_OK;
}

// Which opening a gather workgroup takes.  The openings come in transcript order, i.e. random columns; the tree nodes two
// openings share (every sibling from the level where their columns fall under one parent's two children) and the
// neighbours in a 128-byte line are only read from HBM once if the workgroups that want them run at the same time on
// the SAME XCD (one L2 per XCD).  So: openings sorted by column, and -- workgroup b of a grid row lands on XCD b % 8
// when the row length is a multiple of 8 -- XCD x takes the x-th eighth of the sorted list, in order.
void gather_order(const uint32_t *cols, uint32_t n_cols, uint32_t *order) {
    std::vector<uint32_t> sorted(n_cols);
    for (uint32_t i = 0; i < n_cols; i++) sorted[i] = i;
    std::sort(sorted.begin(), sorted.end(), [cols](uint32_t x, uint32_t y) { return cols[x] != cols[y] ? cols[x] < cols[y] : x < y; });
    if (n_cols % 8 == 0) {
        const uint32_t per = n_cols / 8;
        for (uint32_t b = 0; b < n_cols; b++) order[b] = sorted[(b % 8) * per + b / 8];
    } else {
        memcpy(order, sorted.data(), (size_t)n_cols * 4);
    }
}

// cols_dv: DEVICE pointer (already staged).  Emits the openings of rows [row_lo, row_hi).
// `first_opening`: cols_dv points at opening number first_opening of the list the handle was hinted with (a packed
// handle's rank table is indexed by the opening; zip_open_stream emits the list in groups).
int32_t run_open_columns(zip_commitment *c, const uint32_t *cols_dv, uint32_t n_cols, uint8_t *out_d,
                         uint32_t row_lo, uint32_t row_hi, uint32_t first_opening = 0, hipStream_t st = nullptr,
                         bool alone = false) {
    zip_ctx *ctx = c->ctx;
    if (!st) st = ctx->stream;
    if (n_cols == 0 || row_hi <= row_lo) return ZIP_OK;
    OpenColsArgs a{};
    a.rows = c->rows;
    a.compact_rows = c->compact_rows ? 1u : 0u;
    a.layers = reinterpret_cast<const uint64_t *>(c->layers);
    a.cols = cols_dv;
    a.order = c->gather_order;
    if (c->packed) {
        if (!c->rank_d) return fail(ctx, ZIP_ERR_INVALID_PARAM, "packed commitment without its rank table");
        a.pk = reinterpret_cast<const uint8_t *>(c->rows);
        a.pk_stride = c->pk_stride;
        a.pk_off0 = c->pk_off[0];
        a.pk_off1 = c->pk_off[1];
        a.pk_off2 = c->pk_off[2];
        a.pk_rank = c->rank_d + (size_t)first_opening * 4;
        if (first_opening == 0 && c->plan && n_cols == c->plan->cols.size()) a.wg_tab = c->gather_tab;
    }
    a.out = out_d;
    a.num_rows = ctx->rows_local;
    a.cw = ctx->p.codeword_len;
    a.depth = ctx->depth;
    a.k_limbs = ctx->p.k_limbs;
    a.row_lo = row_lo;
    a.row_hi = row_hi;
    // Rows per workgroup: 32, or fewer where the LDS image of 32 path records would not fit beside the persistent
    // commit workgroups of this geometry -- the gather is meant to run BESIDE them (at cw = 16384 the commit kernel
    // leaves 11.5 KB per CU and 32 records are 14.6 KB: the gathers then only started when the commit ended).
    // (ZIP_HIP_GATHER_RPB: a test hook; each path below takes it only within its own range)
    const uint32_t knob_rpb = ctx->knob_rpb;  // (zip_ctx_create reads it)
    uint32_t rpb = 32u;
    const size_t rec = 8 + 32 * (size_t)ctx->depth;  // bytes of one record in the LDS image
    size_t free_lds = 0;
    {
        const CommitGeom cg = commit_geom(ctx->p.codeword_len, ctx->p.row_len);
        const size_t used = (size_t)commit_wgs_per_cu(cg) * cg.lds;
        free_lds = used < 160u * 1024u ? 160u * 1024u - used : 0;
    }
    if (knob_rpb >= 2 && knob_rpb <= 128) {
        rpb = knob_rpb & ~1u;  // even; the value copy needs <= 128
    } else {
        // (2.5 KB of slack: LDS is handed out in granules -- 24 records = 10.7 KB did NOT get in beside 148.8 KB)
        while (rpb > 8 && rpb * rec + 2560 > free_lds) rpb -= 8;
        // the LAST chunk's gather runs after the commit kernel has ended, with the CU's whole LDS.  On the natural layout 96
        // records per workgroup moved more bytes per workgroup lifetime (0.735 against 0.825 ms for 4096 rows alone at
        // 2^24, round 3) -- unless another job is in flight on the ctx (zip_commit_open_begin: the NEXT job's commit kernel
        // is then resident when this gather runs, and 40 KB of LDS would wait for that kernel to end).  The row-interleaved
        // gather of a packed handle is the other way round: alone, 32 rows per workgroup take 0.094 ms per launch, 64
        // 0.106, 96 0.120, 128 0.166 (measured by a script since removed: EXPERIMENTS.md), and the step ends 27 us
        // sooner with 32 for the last chunk too (1.559-1.561 against 1.580-1.594 ms, alternated three times): no bump.
        if (alone && !c->packed && rpb == 32 && row_hi - row_lo >= 96 && 96 * rec <= 48u * 1024u && !(ctx->job_busy[0] || ctx->job_busy[1])) rpb = 96;
    }
    a.rows_per_block = (row_hi - row_lo) < rpb ? (row_hi - row_lo) : rpb;
    a.prio = 1;
    // Where the commit kernel leaves little LDS (cw = 16384: 16 records per workgroup):
    // the kernel without an LDS image.  ZIP_HIP_GATHER_STREAM=1 / 0 forces it on / off.
    const int knob_stream = ctx->knob_stream;  // (zip_ctx_create reads it)
    const bool stream = knob_stream >= 0 ? knob_stream == 1 : rpb < 32;
    if (c->packed) {
        // a packed commitment: everything row-interleaved in groups of four (open_columns_ilv_kernel); blocks of whole
        // groups
        if (stream) {
            const uint32_t want = (knob_rpb >= 4 && knob_rpb <= 4096) ? (knob_rpb & ~3u) : 32u;
            a.rows_per_block = want;
            const dim3 grid(n_cols, (row_hi - row_lo + a.rows_per_block - 1) / a.rows_per_block), block(256);
            LaunchTimer t(ctx, "open_columns_kernel", st);
            if (want == 64) hipLaunchKernelGGL((open_columns_ilv_kernel<false, 2>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((open_columns_ilv_kernel<false, 1>), grid, block, 0, st, a);
            HIP_TRY(ctx, hipGetLastError());
            return ZIP_OK;
        }
        a.rows_per_block = (rpb + 3u) & ~3u;
        const size_t lds = (size_t)a.rows_per_block * rec;
        const dim3 grid(n_cols, (row_hi - row_lo + a.rows_per_block - 1) / a.rows_per_block), block(256);
        // Every block 32 / 64 whole rows and the launch has its table: the kernel whose addressing stays on the scalar
        // unit (open_columns_ilv_scalar_kernel).  Its lane offsets are 32-bit (a block's span of the packed block must
        // fit), its copy-out is 16-byte stores only, and the depth is a template argument.
        if (a.wg_tab && (a.rows_per_block == 32 || a.rows_per_block == 64) && ctx->depth >= 12 && ctx->depth <= 14 &&
            row_lo % 4 == 0 && (row_hi - row_lo) % a.rows_per_block == 0 && a.num_rows % 2 == 0 &&
            (reinterpret_cast<uintptr_t>(out_d) & 15) == 0 && (uint64_t)a.rows_per_block * a.pk_stride < (1ull << 31)) {
            void (*kern)(OpenColsArgs) = nullptr;
            const bool two = a.rows_per_block == 64;
            switch (ctx->depth) {
                case 12: kern = two ? open_columns_ilv_scalar_kernel<2, 12> : open_columns_ilv_scalar_kernel<1, 12>; break;
                case 13: kern = two ? open_columns_ilv_scalar_kernel<2, 13> : open_columns_ilv_scalar_kernel<1, 13>; break;
                default: kern = two ? open_columns_ilv_scalar_kernel<2, 14> : open_columns_ilv_scalar_kernel<1, 14>; break;
            }
            if (int32_t rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), lds)) return rc;
            LaunchTimer t(ctx, "open_columns_kernel", st);
            hipLaunchKernelGGL(kern, grid, block, lds, st, a);
            HIP_TRY(ctx, hipGetLastError());
            return ZIP_OK;
        }
        // (blocks of 32 / 64 whole rows take the kernel's branch-free path: P passes of 32 rows with all loads in flight)
        const void *fn = a.rows_per_block == 64 ? reinterpret_cast<const void *>(open_columns_ilv_kernel<true, 2>)
                                                : reinterpret_cast<const void *>(open_columns_ilv_kernel<true, 1>);
        if (int32_t rc = ensure_dynamic_lds(ctx, fn, lds)) return rc;
        LaunchTimer t(ctx, "open_columns_kernel", st);
        if (a.rows_per_block == 64) hipLaunchKernelGGL((open_columns_ilv_kernel<true, 2>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((open_columns_ilv_kernel<true, 1>), grid, block, lds, st, a);
        HIP_TRY(ctx, hipGetLastError());
        return ZIP_OK;
    }
    // (A gather with the fewest memory instructions, many rows per workgroup and no LDS, was measured and removed:
    // beside the commit kernel it was the slower choice, 1.92-2.01 against 1.80-1.85 ms per step -- what a gather costs
    // the hashing waves is its VECTOR-MEMORY instructions, not its VALU ones (EXPERIMENTS.md).)
    if (stream && ctx->depth >= 1 && 2 * ctx->depth + 3 <= 64) {
        const uint32_t want = (knob_rpb >= 2 && knob_rpb <= 4096) ? knob_rpb : 32u;
        a.rows_per_block = (row_hi - row_lo) < want ? (row_hi - row_lo) : want;
        const dim3 grid(n_cols, (row_hi - row_lo + a.rows_per_block - 1) / a.rows_per_block), block(256);
        LaunchTimer t(ctx, "open_columns_kernel", st);
        if (2 * ctx->depth + 3 <= 32)
            hipLaunchKernelGGL(open_columns_stream_kernel<32>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(open_columns_stream_kernel<64>, grid, block, 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
        return ZIP_OK;
    }
    const size_t lds = (size_t)a.rows_per_block * (8 + 32 * (size_t)ctx->depth);
    const dim3 grid(n_cols, (row_hi - row_lo + a.rows_per_block - 1) / a.rows_per_block), block(256);
    LaunchTimer t(ctx, "open_columns_kernel", st);
    if (2 * ctx->depth + 1 <= 32)
        hipLaunchKernelGGL(open_columns_kernel<32>, grid, block, lds, st, a);
    else
        hipLaunchKernelGGL(open_columns_kernel<64>, grid, block, lds, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

// All chunks, each gated on the arrival counter of the (possibly still running) persistent
// commit kernel: the memory-bound gather of chunk k runs beside the hashing of later chunks.
int32_t run_open_columns_pipelined(zip_commitment *c, const uint32_t *cols_dv, uint32_t n_cols, uint8_t *out_d) {
    zip_ctx *ctx = c->ctx;
    if (!c->chunk_done || (c->ring_slot && c->ring_epoch != ctx->ring_epoch)) {
        int32_t rc = wait_ready(c, ctx->stream);
        if (rc) return rc;
        return run_open_columns(c, cols_dv, n_cols, out_d, 0, ctx->rows_local, 0, nullptr, /*alone=*/true);
    }
    if (c->zeroed) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, c->zeroed, 0));
    // The gathers of consecutive chunks do not depend on each other, only each on ITS chunk, but they stay on one
    // stream: alternating two streams was measured WORSE (round 3), 1.96-2.00 against 1.88 ms per step on one box --
    // gathers that overlap each other take longer in sum and slow the commit kernel more (path removed: EXPERIMENTS.md).
    // test hook: an unreachable target and a 1 ms limit exercise the recovery path of a timed-out wait
    // (a value > 1 is the limit in ticks of the 100 MHz clock: short enough and the gathers run BEFORE their rows exist)
    const bool force_timeout = getenv("ZIP_HIP_FORCE_WAIT_TIMEOUT") != nullptr;
    const unsigned long long force_ticks = (unsigned long long)env_long("ZIP_HIP_FORCE_WAIT_TIMEOUT", 100000, 2, LONG_MAX);
    auto wait_for = [&](hipStream_t st, uint32_t *counter, uint32_t target) -> int32_t {
        LaunchTimer t(ctx, "wait_counter_kernel", st);
        hipLaunchKernelGGL(wait_counter_kernel, dim3(1), dim3(64), 0, st, counter, force_timeout ? 0xFFFFFFFFu : target, 0u,
                           ctx->timeout_flag_d, force_timeout ? force_ticks : 25000000ull /* 0.25 s at 100 MHz */);
        HIP_TRY(ctx, hipGetLastError());
        return ZIP_OK;
    };
    for (size_t k = 0; k + 1 < c->bounds.size(); k++) {
        int32_t rc = wait_for(ctx->stream, c->chunk_done + k, c->expected[k]);
        if (rc) return rc;
        rc = run_open_columns(c, cols_dv, n_cols, out_d, c->bounds[k], c->bounds[k + 1], 0, ctx->stream,
                              /*alone=*/k + 2 == c->bounds.size());
        if (rc) return rc;
    }
    return ZIP_OK;
}

size_t column_bytes(const zip_ctx *ctx) {
    return (size_t)ctx->rows_local * (8 * (size_t)ctx->p.k_limbs + 8 + 32 * (size_t)ctx->depth);
}

// A wait of the pipelined gather gave up: its stream was parked on a chunk counter while the commit
// kernel could not run -- which happens when something serialises kernel dispatch across streams
// (rocprofv3 counter collection does, and may run the waiter first).  The gathers behind that wait
// read rows that did not exist yet, so the whole gather is redone once the commit has really finished.
// `force`: redo it although the flag is down -- another job's recovery has already drained the stream and cleared the
// flag, and THIS job's gathers may have run behind a timed-out wait as well (zip_job_wait, two jobs in flight).
int32_t recover_gather_timeout(zip_commitment *c, const uint32_t *cols_dv, uint32_t n_cols, uint8_t *out_d, bool force = false) {
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, stream_wait(ctx->stream));
    const bool timed_out = ctx->timeout_flag_h && *ctx->timeout_flag_h;
    if (!timed_out && !force) return ZIP_OK;
    if (timed_out) ctx->recover_epoch++;
    if (ctx->timeout_flag_h) *ctx->timeout_flag_h = 0;
    int32_t rc = wait_ready(c, ctx->stream);
    if (rc) return rc;
    if ((rc = run_open_columns(c, cols_dv, n_cols, out_d, 0, ctx->rows_local))) return rc;
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

// a raised timeout flag nobody recovered from is an error
int32_t check_timeout(zip_ctx *ctx) {
    if (ctx->timeout_flag_h && *ctx->timeout_flag_h) {
        *ctx->timeout_flag_h = 0;
        return fail(ctx, ZIP_ERR_HIP, "a pipeline stage waited for the commit kernel and gave up");
    }
    return ZIP_OK;
}

// copies a device result to the caller's buffer (host: synchronous)
int32_t deliver(zip_ctx *ctx, void *dst, zip_mem_kind kind, const void *src_d, size_t bytes) {
    if (kind == ZIP_MEM_HOST) {
        int32_t rc = copy_d2h_bounced(ctx, dst, src_d, bytes, ctx->stream);
        if (rc) return rc;
        return check_timeout(ctx);
    } else if (dst != src_d) {
        HIP_TRY(ctx, hipMemcpyAsync(dst, src_d, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return ZIP_OK;
}


// ------------------------------------------------------------------ verifier side
// Montgomery constants of 2^256 - q, the modulus the reference actually reduces Int<4> column
// entries by when q has its top bit set in four limbs (field_from_int256 in kernels_verify.cuh).
bool make_quirk_field(const HostField &hf, HostField *fq) {
    if (hf.fl != 4 || !(hf.modulus[3] >> 63)) return false;
    uint64_t m[8] = {0};
    sub_limbs(m, hf.modulus, 4);  // 2^256 - q (odd, < 2^255)
    fq->fl = 4;
    memcpy(fq->modulus, m, 32);
    uint64_t inv = 1;
    for (int i = 0; i < 63; i++) {
        inv *= inv;
        inv *= m[0];
    }
    fq->inv = (uint64_t)0 - inv;
    // R mod q' and R^2 mod q' by doubling; start from 1 mod q' (q' may be 1: then everything is 0)
    bool one = m[0] == 1 && !m[1] && !m[2] && !m[3];
    uint64_t x[8] = {one ? 0ull : 1ull};
    for (uint32_t i = 0; i < 256; i++) dbl_mod(x, m, 4);
    memcpy(fq->r, x, 32);
    for (uint32_t i = 0; i < 256; i++) dbl_mod(x, m, 4);
    memcpy(fq->r2, x, 32);
    fq->quirk_mod = 0;
    return true;
}

// FieldDev of the field and of 2^256 - q for the verifier's kernels (fq = fd and quirk = 0 unless the quirk applies)
template <int FL>
struct VerifyField {
    FieldDev<FL> fd, fq;
    uint32_t quirk;
};
template <int FL>
VerifyField<FL> verify_field(const HostField &hf) {
    VerifyField<FL> v{to_dev<FL>(hf), to_dev<FL>(hf), 0u};
    if constexpr (FL == 4) {
        HostField hq;
        if (make_quirk_field(hf, &hq)) {
            v.fq = to_dev<4>(hq);
            v.quirk = 1u;
        }
    }
    return v;
}

// The encoders' workgroup: one thread per codeword element up to 1024, at least a wave (a power of two: the batch
// kernel's dot-product tree needs one), and one element of dynamic LDS per thread.
struct EncodeShape {
    uint32_t threads;
    size_t lds;
};
template <int L, bool FIELD>
EncodeShape encode_shape(uint32_t cw) {
    const uint32_t threads = cw < 1024 ? (cw < 64 ? 64 : cw) : 1024;
    return {threads, (size_t)threads * sizeof(EncElem<L, FIELD>)};
}

template <int L, bool FIELD>
int32_t launch_encode_row(zip_ctx *ctx, const uint64_t *in, uint64_t *tmp, uint64_t *out, const FieldDev<L> &fd,
                          uint32_t *overflow) {
    const EncodeShape s = encode_shape<L, FIELD>(ctx->p.codeword_len);
    auto kern = encode_row_kernel<L, FIELD>;
    if (int32_t rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), s.lds)) return rc;
    LaunchTimer t(ctx, "encode_row_kernel");
    hipLaunchKernelGGL(kern, dim3(1), dim3(s.threads), s.lds, ctx->stream, in, ctx->p.row_len, ctx->p.codeword_len, ctx->perm1_d,
                       ctx->perm2_d, tmp, out, fd, overflow);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

// the device inputs of zip_verify (n_polys = 1, no evals_d) and zip_batch_verify
struct VerifyIn {
    const uint8_t *proofs_d;
    size_t stream_bytes;
    const uint8_t *roots_d;
    const int64_t *coeffs_d;
    const uint32_t *cols_d;
    const uint64_t *q0_d, *q1_d, *evals_d;
    uint32_t n_cols, n_polys;
};

// What zip_verify and zip_batch_verify ask of their arguments alike; n_openings: over all the proofs
int32_t check_verify_args(zip_ctx *ctx, const int64_t *coeffs, const uint32_t *cols, uint32_t n_openings, const uint64_t *q0_mont,
                          const uint64_t *q1_mont, const zip_field *field, HostField *hf) {
    if (int32_t rc = make_field(ctx, field, hf)) return rc;
    if (ctx->p.num_rows > 1 && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if (ctx->p.row_len > 1 && !q1_mont) return fail(ctx, ZIP_ERR_NULL, "q1_mont is NULL");
    return check_cols(ctx, cols, n_openings);
}

// k proof streams to the device when they are the host's, and the small inputs of k proofs in one block.
// q_1 of a one-column matrix is empty in the reference (pcs/utils.rs:253-276): <row, q1> is then 0.
int32_t stage_verify_inputs(zip_ctx *ctx, uint32_t k, size_t stream_bytes, const uint8_t *proofs, zip_mem_kind proofs_kind,
                            const uint8_t *roots, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols,
                            const uint64_t *q0_mont, const uint64_t *q1_mont, const uint64_t *evals_mont, uint32_t fl,
                            Scratch &pbuf, Scratch &small, VerifyIn *in, uint32_t n_tests = 1) {
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len;
    const bool single = R == 1;
    int32_t rc;
    in->proofs_d = proofs;
    if (proofs_kind == ZIP_MEM_HOST) {
        if ((rc = pbuf.get((size_t)k * stream_bytes))) return rc;
        if ((rc = copy_h2d_bounced(ctx, pbuf.ptr, proofs, (size_t)k * stream_bytes, ctx->stream))) return rc;
        in->proofs_d = pbuf.as<uint8_t>();
    }
    SmallInputs si;
    si.src[0] = coeffs;     si.bytes[0] = single ? 0 : (size_t)k * n_tests * R * 8;  // (n_tests > 1: zip_verify, k = 1)
    si.src[1] = q0_mont;    si.bytes[1] = single ? 0 : (size_t)k * R * fl * 8;
    si.src[2] = cols;       si.bytes[2] = (size_t)k * n_cols * 4;
    si.src[3] = q1_mont;    si.bytes[3] = C > 1 ? (size_t)k * C * fl * 8 : 0;
    si.src[4] = roots;      si.bytes[4] = (size_t)k * R * 32;
    si.src[5] = evals_mont; si.bytes[5] = evals_mont ? (size_t)k * fl * 8 : 0;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    in->stream_bytes = stream_bytes;
    in->coeffs_d = reinterpret_cast<const int64_t *>(sb + si.off[0]);
    in->q0_d = reinterpret_cast<const uint64_t *>(sb + si.off[1]);
    in->cols_d = reinterpret_cast<const uint32_t *>(sb + si.off[2]);
    in->q1_d = reinterpret_cast<const uint64_t *>(sb + si.off[3]);
    in->roots_d = sb + si.off[4];
    in->evals_d = reinterpret_cast<const uint64_t *>(sb + si.off[5]);
    in->n_cols = n_cols;
    in->n_polys = k;
    return ZIP_OK;
}

template <int FL>
int32_t run_verify_fl(zip_ctx *ctx, const VerifyIn &in, const HostField &hf, std::vector<uint32_t> &flags,
                      std::vector<uint32_t> &bad, std::vector<uint32_t> &malformed, VerifyHead *cnt) {
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, cw = ctx->p.codeword_len, M = ctx->p.m_limbs;
    const uint32_t n_cols = in.n_cols;
    const bool single = R == 1;
    const uint32_t T = proximity_tests(ctx);   // u'_0 .. u'_{T-1} head the stream; coeffs_d is [T][R]
    const size_t u_bytes = uprime_bytes(ctx);
    const size_t cols_bytes = (size_t)n_cols * column_bytes(ctx);
    const uint32_t blocks = (R + 255) / 256;
    Scratch enc_u(ctx), enc_f(ctx), tmp(ctx), row(ctx), parts(ctx), misc(ctx);
    int32_t rc;
    if ((rc = enc_u.get((size_t)T * cw * M * 8))) return rc;  // encode_wide(u'_t), test-major
    if ((rc = enc_f.get((size_t)cw * FL * 8))) return rc;
    if ((rc = tmp.get((size_t)cw * M * 8))) return rc;
    if ((rc = row.get((size_t)C * FL * 8))) return rc;
    if ((rc = parts.get((size_t)n_cols * blocks * (6 + FL) * 8 + 64))) return rc;
    // misc: head | flags[n] | bad[n] | malformed[n], one device block, copied back in one piece
    const size_t misc_bytes = sizeof(VerifyHead) + (size_t)3 * n_cols * 4;
    if ((rc = misc.get(misc_bytes))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(misc.ptr, 0, misc_bytes, ctx->stream));
    VerifyHead *cnt_d = misc.as<VerifyHead>();
    uint32_t *flags_d = reinterpret_cast<uint32_t *>(cnt_d + 1), *bad_d = flags_d + n_cols, *mal_d = bad_d + n_cols;
    const VerifyField<FL> vf = verify_field<FL>(hf);
    const FieldDev<FL> &fd = vf.fd;
    // encode_wide(u') (verify_z.rs:75-77)
    if (!single) {
        FieldDev<8> unused{};
        // (per test, one after the other on the stream: they share `tmp`; an overflow in any test is the one fact)
        for (uint32_t t = 0; t < T; t++)
            if ((rc = launch_encode_row<8, false>(ctx, reinterpret_cast<const uint64_t *>(in.proofs_d) + (size_t)t * C * M,
                                                  tmp.as<uint64_t>(), enc_u.as<uint64_t>() + (size_t)t * cw * M, unused,
                                                  &cnt_d->overflow)))
                return rc;
    }
    // read_field_elements + encode_f + <row, q1> (verify_z.rs:139-149)
    {
        LaunchTimer t(ctx, "decode_field_row_kernel");
        hipLaunchKernelGGL(decode_field_row_kernel<FL>, dim3((C + 255) / 256), dim3(256), 0, ctx->stream,
                           in.proofs_d + u_bytes + cols_bytes, C, row.as<uint64_t>(), &cnt_d->noncanonical, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    if ((rc = launch_encode_row<FL, true>(ctx, row.as<uint64_t>(), tmp.as<uint64_t>(), enc_f.as<uint64_t>(), fd, nullptr)))
        return rc;
    {
        LaunchTimer t(ctx, "field_dot_kernel");
        hipLaunchKernelGGL(field_dot_kernel<FL>, dim3(1), dim3(1024), 0, ctx->stream, row.as<uint64_t>(), in.q1_d, C,
                           cnt_d->dot, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (n_cols) {
        VerifyColsArgs a{};
        a.wire = in.proofs_d + u_bytes;
        a.cols = in.cols_d;
        a.coeffs = single ? nullptr : in.coeffs_d;
        a.q0 = single ? nullptr : in.q0_d;
        a.roots = reinterpret_cast<const uint32_t *>(in.roots_d);
        a.num_rows = R;
        a.depth = ctx->depth;
        a.n_cols = n_cols;
        a.quirk = vf.quirk;
        a.part_int = parts.as<uint64_t>();
        a.part_f = a.part_int + (size_t)n_cols * blocks * 6;
        a.bad_merkle = bad_d;
        a.malformed = mal_d;
        {
            LaunchTimer t(ctx, "verify_columns_kernel");
            hipLaunchKernelGGL(verify_columns_kernel<FL>, dim3(n_cols, blocks), dim3(256), 0, ctx->stream, a, fd, vf.fq);
            HIP_TRY(ctx, hipGetLastError());
        }
        {
            LaunchTimer t(ctx, "verify_finalize_kernel");
            hipLaunchKernelGGL(verify_finalize_kernel<FL>, dim3((n_cols + 255) / 256), dim3(256), 0, ctx->stream,
                               a.part_int, a.part_f, blocks, in.cols_d, n_cols,
                               single ? nullptr : enc_u.as<uint64_t>(), M, enc_f.as<uint64_t>(), flags_d, fd);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (T > 1) {  // tests 1 .. T-1 of every opening: bit 0 becomes "any test failed here" (verify_z.rs:92-97)
            VerifyExtraArgs x{};
            x.wire = a.wire;
            x.cols = in.cols_d;
            x.coeffs = in.coeffs_d + R;
            x.enc_u = enc_u.as<uint64_t>() + (size_t)cw * M;
            x.num_rows = R;
            x.depth = ctx->depth;
            x.n_cols = n_cols;
            x.cw = cw;
            x.m_limbs = M;
            x.n_tests = T - 1;
            x.flags = flags_d;
            LaunchTimer t(ctx, "verify_extra_tests_kernel");
            hipLaunchKernelGGL(verify_extra_tests_kernel, dim3(n_cols), dim3(256), 0, ctx->stream, x);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    std::vector<unsigned char> host(misc_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), misc.ptr, misc_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    memcpy(cnt, host.data(), sizeof(VerifyHead));
    const uint32_t *w = reinterpret_cast<const uint32_t *>(host.data() + sizeof(VerifyHead));
    flags.assign(w, w + n_cols);
    bad.assign(w + n_cols, w + 2 * n_cols);
    malformed.assign(w + 2 * n_cols, w + 3 * n_cols);
    return ZIP_OK;
}

// ---- the batched verifier (zip_batch_verify): five launches whatever n_polys is -- encode_wide(u'), encode_f(row) with
// the decode and <row, q1> fused in, the column checks, the reports -- one device-to-host copy of n_polys reports, one wait.

// Process-wide count of zip_batch_verify calls that reached the device (zip_batch_verify_calls)
std::atomic<uint64_t> g_batch_verify_calls{0};

template <int L, bool FIELD>
int32_t launch_batch_encode(zip_ctx *ctx, BatchEncodeArgs a, uint32_t n_polys, const FieldDev<L> &fd, const char *name) {
    const EncodeShape s = encode_shape<L, FIELD>(ctx->p.codeword_len);
    auto kern = batch_encode_kernel<L, FIELD>;
    if (int32_t rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), s.lds)) return rc;
    LaunchTimer t(ctx, name);
    hipLaunchKernelGGL(kern, dim3(n_polys), dim3(s.threads), s.lds, ctx->stream, a, fd);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

template <int FL>
int32_t run_batch_verify_fl(zip_ctx *ctx, const VerifyIn &in, const HostField &hf, zip_verify_report *reports) {
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, cw = ctx->p.codeword_len, M = ctx->p.m_limbs;
    const uint32_t n_cols = in.n_cols, B = in.n_polys;
    const bool single = R == 1;
    const size_t u_bytes = single ? 0 : (size_t)C * M * 8;
    const size_t cols_bytes = (size_t)n_cols * column_bytes(ctx);
    Scratch enc_u(ctx), enc_f(ctx), tmp(ctx), misc(ctx);
    int32_t rc;
    if (!single && (rc = enc_u.get((size_t)B * cw * M * 8))) return rc;
    if ((rc = enc_f.get((size_t)B * cw * FL * 8))) return rc;
    if ((rc = tmp.get((size_t)B * cw * (single ? FL : M) * 8))) return rc;  // (the two encodings run one after the other)
    // misc: reports[B] | heads[B] | flags[B n] | bad[B n] | malformed[B n]; every word is written before it is read
    const size_t per_opening = (size_t)B * n_cols * 4;
    const size_t misc_bytes = (size_t)B * (sizeof(zip_verify_report) + sizeof(VerifyHead)) + 3 * per_opening;
    if ((rc = misc.get(misc_bytes))) return rc;
    zip_verify_report *reports_d = misc.as<zip_verify_report>();
    VerifyHead *head_d = reinterpret_cast<VerifyHead *>(reports_d + B);
    uint32_t *flags_d = reinterpret_cast<uint32_t *>(head_d + B), *bad_d = flags_d + (size_t)B * n_cols,
             *mal_d = bad_d + (size_t)B * n_cols;
    const VerifyField<FL> vf = verify_field<FL>(hf);
    const FieldDev<FL> &fd = vf.fd;
    BatchEncodeArgs e{};
    e.proofs = in.proofs_d;
    e.stream_bytes = in.stream_bytes;
    e.row_len = C;
    e.cw = cw;
    e.perm1 = ctx->perm1_d;
    e.perm2 = ctx->perm2_d;
    e.tmp = tmp.as<uint64_t>();
    e.head = head_d;
    if (!single) {  // encode_wide(u') (verify_z.rs:75-77)
        FieldDev<8> unused{};
        e.in_at = 0;
        e.out = enc_u.as<uint64_t>();
        if ((rc = launch_batch_encode<8, false>(ctx, e, B, unused, "batch_encode_wide_kernel"))) return rc;
    }
    // read_field_elements + encode_f + <row, q1> (verify_z.rs:139-149)
    e.in_at = u_bytes + cols_bytes;
    e.out = enc_f.as<uint64_t>();
    e.q1 = C > 1 ? in.q1_d : nullptr;
    e.clear_overflow = single ? 1u : 0u;
    if ((rc = launch_batch_encode<FL, true>(ctx, e, B, fd, "batch_encode_field_kernel"))) return rc;
    if (n_cols) {
        BatchVerifyColsArgs a{};
        a.proofs = in.proofs_d;
        a.stream_bytes = in.stream_bytes;
        a.openings_at = u_bytes;
        a.cols = in.cols_d;
        a.coeffs = single ? nullptr : in.coeffs_d;
        a.q0 = single ? nullptr : in.q0_d;
        a.roots = reinterpret_cast<const uint32_t *>(in.roots_d);
        a.enc_u = single ? nullptr : enc_u.as<uint64_t>();
        a.enc_f = enc_f.as<uint64_t>();
        a.num_rows = R;
        a.depth = ctx->depth;
        a.n_cols = n_cols;
        a.cw = cw;
        a.quirk = vf.quirk;
        a.flags = flags_d;
        a.bad_merkle = bad_d;
        a.malformed = mal_d;
        const uint32_t per_wg = R < 256 ? 256 / R : 1;  // openings per workgroup
        LaunchTimer t(ctx, "batch_verify_columns_kernel");
        hipLaunchKernelGGL(batch_verify_columns_kernel<FL>, dim3((n_cols + per_wg - 1) / per_wg, B), dim3(256), 0, ctx->stream, a, fd, vf.fq);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        BatchVerifyReportArgs a{};
        a.flags = flags_d;
        a.bad_merkle = bad_d;
        a.malformed = mal_d;
        a.head = head_d;
        a.evals = in.evals_d;
        a.n_cols = n_cols;
        a.row_len = C;
        a.reports = reports_d;
        LaunchTimer t(ctx, "batch_verify_report_kernel");
        hipLaunchKernelGGL(batch_verify_report_kernel<FL>, dim3(B), dim3(256), 0, ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(reports, reports_d, (size_t)B * sizeof(zip_verify_report), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

// ---- zip_batch_verify_codes: the same five launches with a code and a field per member (BatchVerifyMember) ----
// Process-wide (zip_batch_verify_codes_counts): calls that reached the device, and the members they verified
std::atomic<uint64_t> g_batch_verify_codes_calls{0}, g_batch_verify_codes_members{0};

// BatchVerifyMember<FL>[k]: member i's field, the start of its stream and its slices of the uploaded permutations
template <int FL>
void batch_fill_verify_members(const std::vector<HostField> &hf, const std::vector<const uint8_t *> &streams, const uint32_t *perms1_d,
                               const uint32_t *perms2_d, uint32_t cw, std::vector<unsigned char> *inst) {
    inst->assign(hf.size() * sizeof(BatchVerifyMember<FL>), 0);
    BatchVerifyMember<FL> *m = reinterpret_cast<BatchVerifyMember<FL> *>(inst->data());
    for (size_t i = 0; i < hf.size(); i++) {
        const VerifyField<FL> vf = verify_field<FL>(hf[i]);
        m[i].f = vf.fd;
        m[i].fq = vf.fq;
        m[i].quirk = vf.quirk;
        m[i].stream = streams[i];
        m[i].perm1 = perms1_d + i * cw;
        m[i].perm2 = perms2_d + i * cw;
    }
}

// in.proofs_d / in.stream_bytes are not read: the streams are the entries' (inst_d: BatchVerifyMember<FL>[in.n_polys])
template <int FL>
int32_t run_batch_verify_codes_fl(zip_ctx *ctx, const VerifyIn &in, const void *inst_d, zip_verify_report *reports) {
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, cw = ctx->p.codeword_len, M = ctx->p.m_limbs;
    const uint32_t n_cols = in.n_cols, B = in.n_polys;
    const bool single = R == 1;
    const size_t u_bytes = single ? 0 : (size_t)C * M * 8;
    const size_t cols_bytes = (size_t)n_cols * column_bytes(ctx);
    const BatchVerifyMember<FL> *inst = static_cast<const BatchVerifyMember<FL> *>(inst_d);
    Scratch enc_u(ctx), enc_f(ctx), tmp(ctx), misc(ctx);
    int32_t rc;
    if (!single && (rc = enc_u.get((size_t)B * cw * M * 8))) return rc;
    if ((rc = enc_f.get((size_t)B * cw * FL * 8))) return rc;
    if ((rc = tmp.get((size_t)B * cw * (single ? FL : M) * 8))) return rc;
    // misc: as in run_batch_verify_fl
    const size_t per_opening = (size_t)B * n_cols * 4;
    const size_t misc_bytes = (size_t)B * (sizeof(zip_verify_report) + sizeof(VerifyHead)) + 3 * per_opening;
    if ((rc = misc.get(misc_bytes))) return rc;
    zip_verify_report *reports_d = misc.as<zip_verify_report>();
    VerifyHead *head_d = reinterpret_cast<VerifyHead *>(reports_d + B);
    uint32_t *flags_d = reinterpret_cast<uint32_t *>(head_d + B), *bad_d = flags_d + (size_t)B * n_cols,
             *mal_d = bad_d + (size_t)B * n_cols;
    BatchEncodeArgs e{};
    e.row_len = C;
    e.cw = cw;
    e.tmp = tmp.as<uint64_t>();
    e.head = head_d;
    if (!single) {  // encode_wide(u')
        const EncodeShape s = encode_shape<8, false>(cw);
        auto kern = batch_encode_codes_kernel<8, false, FL>;
        if ((rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), s.lds))) return rc;
        e.in_at = 0;
        e.out = enc_u.as<uint64_t>();
        LaunchTimer t(ctx, "batch_encode_wide_codes_kernel");
        hipLaunchKernelGGL(kern, dim3(B), dim3(s.threads), s.lds, ctx->stream, e, inst);
        HIP_TRY(ctx, hipGetLastError());
    }
    {   // read_field_elements + encode_f + <row, q1>
        const EncodeShape s = encode_shape<FL, true>(cw);
        auto kern = batch_encode_codes_kernel<FL, true, FL>;
        if ((rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), s.lds))) return rc;
        e.in_at = u_bytes + cols_bytes;
        e.out = enc_f.as<uint64_t>();
        e.q1 = C > 1 ? in.q1_d : nullptr;
        e.clear_overflow = single ? 1u : 0u;
        LaunchTimer t(ctx, "batch_encode_field_codes_kernel");
        hipLaunchKernelGGL(kern, dim3(B), dim3(s.threads), s.lds, ctx->stream, e, inst);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (n_cols) {
        BatchVerifyColsArgs a{};
        a.openings_at = u_bytes;
        a.cols = in.cols_d;
        a.coeffs = single ? nullptr : in.coeffs_d;
        a.q0 = single ? nullptr : in.q0_d;
        a.roots = reinterpret_cast<const uint32_t *>(in.roots_d);
        a.enc_u = single ? nullptr : enc_u.as<uint64_t>();
        a.enc_f = enc_f.as<uint64_t>();
        a.num_rows = R;
        a.depth = ctx->depth;
        a.n_cols = n_cols;
        a.cw = cw;
        a.flags = flags_d;
        a.bad_merkle = bad_d;
        a.malformed = mal_d;
        const uint32_t per_wg = R < 256 ? 256 / R : 1;  // openings per workgroup
        LaunchTimer t(ctx, "batch_verify_columns_codes_kernel");
        hipLaunchKernelGGL(batch_verify_columns_codes_kernel<FL>, dim3((n_cols + per_wg - 1) / per_wg, B), dim3(256), 0, ctx->stream, a, inst);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        BatchVerifyReportArgs a{};
        a.flags = flags_d;
        a.bad_merkle = bad_d;
        a.malformed = mal_d;
        a.head = head_d;
        a.evals = in.evals_d;
        a.n_cols = n_cols;
        a.row_len = C;
        a.reports = reports_d;
        LaunchTimer t(ctx, "batch_verify_report_kernel");
        hipLaunchKernelGGL(batch_verify_report_kernel<FL>, dim3(B), dim3(256), 0, ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(reports, reports_d, (size_t)B * sizeof(zip_verify_report), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

}  // namespace

// ---- sumcheck prover -----------------------------------------
namespace {
// Process-wide counts of the regime the round-kernel launches ran in (zip_sumcheck_grid_counts): computed here, on
// the host, from the points of the round, the final grid and the kernel's points per workgroup
std::atomic<uint64_t> g_sumcheck_multi_pass{0}, g_sumcheck_uneven_last_pass{0}, g_sumcheck_reduce_launches{0};

// The grid of a round-kernel launch after its last cap, and the regime it runs in.  ZIP_HIP_SUMCHECK_GRID=n (test hook,
// 1 .. 8 per CU; per call: the tests flip it) caps the workgroups after the occupancy cap, so that the tests reach several
// passes of the grid-stride loop, an uneven last pass and both reductions at small sizes; unset: `blocks` as it came.
uint32_t sumcheck_final_grid(const zip_sumcheck *s, uint32_t blocks, uint64_t half, uint32_t points_per_wg) {
    blocks = std::min<uint32_t>(blocks, (uint32_t)env_long("ZIP_HIP_SUMCHECK_GRID", (long)s->max_blocks, 1, (long)s->max_blocks));
    const uint64_t worth = (half + points_per_wg - 1) / points_per_wg;  // workgroups' worth of points
    if (worth > blocks) {
        g_sumcheck_multi_pass++;
        if (worth % blocks) g_sumcheck_uneven_last_pass++;
    }
    if (blocks > 64) g_sumcheck_reduce_launches++;
    return blocks;
}

// Workgroups of a round kernel that one CU holds at a time, asked once per (kernel, device).  0: the query failed --
// the caller caps nothing, and the next call asks again.
int sumcheck_round_occupancy(zip_ctx *ctx, const void *kern, size_t lds) {
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, int> occ;
    std::lock_guard<std::mutex> g(mu);
    int &per_cu = occ[std::make_pair(kern, ctx->device)];
    if (per_cu == 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess) per_cu = 0;
    return per_cu;
}

// One round: `kern` over a.half hypercube points, `points_per_wg` of them per workgroup and pass, timed as `name`.
template <int FL, class Args>
int32_t launch_sumcheck_kernel(zip_sumcheck *s, void (*kern)(Args, FieldDev<FL>), const char *name, size_t lds,
                               uint32_t points_per_wg, Args a, const FieldDev<FL> &fd) {
    zip_ctx *ctx = s->ctx;
    const uint64_t want = (a.half + points_per_wg - 1) / points_per_wg;
    uint32_t blocks = (uint32_t)std::min<uint64_t>(want ? want : 1, s->max_blocks);
    // a big round runs as exactly the workgroups that are resident together (grid-stride loop inside): a grid of
    // 8 per CU with 3 resident left a third wave of workgroups two thirds full
    if (blocks > ctx->num_cus) {
        const int per_cu = sumcheck_round_occupancy(ctx, reinterpret_cast<const void *>(kern), lds);
        if (per_cu > 0) blocks = std::min<uint32_t>(blocks, ctx->num_cus * (uint32_t)per_cu);
    }
    blocks = sumcheck_final_grid(s, blocks, a.half, points_per_wg);
    // small rounds: one launch, the last workgroup folds the partials; otherwise sumcheck_reduce_kernel does
    a.done = blocks <= 64 ? s->done_d : nullptr;
    {
        LaunchTimer t(ctx, name);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, ctx->stream, a, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (!a.done) {
        LaunchTimer t(ctx, "sumcheck_reduce_kernel");
        hipLaunchKernelGGL(sumcheck_reduce_kernel<FL>, dim3(1), dim3(256), 0, ctx->stream, a.partials, blocks, a.degree + 1, a.evals_out, fd,
                           a.host_flag, a.seq);
        HIP_TRY(ctx, hipGetLastError());
    }
    return ZIP_OK;
}

template <int FL, int K, int DEG>
int32_t launch_sumcheck_round(zip_sumcheck *s, const SumcheckRoundArgs<FL> &a, const FieldDev<FL> &fd) {
    if constexpr (DEG == 3 || DEG == 2) {
        // Degree 3, the FOLDING rounds (all but the first): there the quad kernel is as fast in the big rounds and up to
        // 1.4x as fast in the small ones (four times the threads for the same number of points, five waves per SIMD
        // instead of two); the first round has no fold to share and pays the point values four times over (1.99 against
        // 1.45 ms at 2^24): it stays on the one-thread-per-point kernel.  Degree 2 (ZincProver's second sumcheck) leaves
        // the fourth lane of a quad idle: slower in the big rounds (0.96 against 0.57 ms in round 2 of 2^24), faster from
        // 2^16 points down (the last rounds: 32 against 49 us).  ZIP_HIP_SUMCHECK_QUAD=0 / 2: never / every round.
        const long mode = env_long("ZIP_HIP_SUMCHECK_QUAD", 1, 0, 2);  // (per call: the tests flip it)
        const bool pays = a.fold && (DEG == 3 || a.half <= 65536u);
        // four lanes per hypercube point (sumcheck_round_quad_kernel, <= 128 VGPRs), 64 points per workgroup
        if (mode == 2 || (mode == 1 && pays))
            return launch_sumcheck_kernel<FL>(s, sumcheck_round_quad_kernel<FL, K, DEG>, "sumcheck_round_kernel", (size_t)256 * FL * 8, 64, a, fd);
    }
    // (extra dynamic LDS to lower the occupancy was an experiment, since removed: EXPERIMENTS.md)
    return launch_sumcheck_kernel<FL>(s, sumcheck_round_kernel<FL, K, DEG>, "sumcheck_round_kernel", (size_t)256 * (DEG + 1) * FL * 8, 256, a, fd);
}

// 5..8 MLEs: eight lanes per hypercube point (sumcheck_round_wide_kernel), every degree and every round; 32 points per
// workgroup.  ZIP_HIP_SUMCHECK_QUAD does not apply here.
template <int FL, int K>
int32_t launch_sumcheck_wide(zip_sumcheck *s, const SumcheckRoundArgs<FL> &a, const FieldDev<FL> &fd) {
    return launch_sumcheck_kernel<FL>(s, sumcheck_round_wide_kernel<FL, K>, "sumcheck_round_wide_kernel", (size_t)256 * FL * 8,
                                      256 / kSumcheckWideLanes, a, fd);
}

template <int FL, int K>
int32_t sumcheck_round_k(zip_sumcheck *s, const SumcheckRoundArgs<FL> &a, const FieldDev<FL> &fd) {
    switch (s->degree) {
        case 1: return launch_sumcheck_round<FL, K, 1>(s, a, fd);
        case 2: return launch_sumcheck_round<FL, K, 2>(s, a, fd);
        case 3: return launch_sumcheck_round<FL, K, 3>(s, a, fd);
        default: return launch_sumcheck_round<FL, K, 4>(s, a, fd);
    }
}

// 0 = general, 1 = one (R), 2 = minus one (q - R): SumcheckRoundArgs::coeff_kind
uint32_t coeff_kind(const uint64_t *coeff, const HostField &hf) {
    uint64_t minus_one[8] = {0};
    memcpy(minus_one, hf.modulus, 8 * (size_t)hf.fl);
    sub_limbs(minus_one, hf.r, hf.fl);  // q - R
    return !cmp_limbs(coeff, hf.r, hf.fl) ? 1u : !cmp_limbs(coeff, minus_one, hf.fl) ? 2u : 0u;
}

// What SumcheckRoundArgs and SumcheckProductsArgs share, for round s->round + 1.  (a.done -- the last workgroup folds the
// partials, or sumcheck_reduce_kernel does -- is the launcher's: it knows the final grid.)
template <int FL, class Args>
void sumcheck_fill_round(const zip_sumcheck *s, const uint64_t *r_prev, Args &a) {
    const HostField &hf = s->field;
    const uint32_t round = s->round + 1;  // 1-based
    a.degree = s->degree;
    a.half = (uint64_t)1 << (s->num_vars - round);
    a.fold = round > 1;
    a.partials = s->partials;
    a.evals_out = s->evals_pinned ? reinterpret_cast<uint64_t *>(s->evals_pinned) : s->evals_d;
    a.host_flag = s->evals_pinned ? reinterpret_cast<uint32_t *>(s->evals_pinned + 192) : nullptr;
    a.seq = round;
    for (uint32_t t = 0; t < s->n_terms; t++) {
        for (int i = 0; i < FL; i++) a.coeff[t][i] = s->coeff[t][i];
        a.coeff_kind[t] = coeff_kind(s->coeff[t], hf);
    }
    for (uint32_t k = 0; k < s->n_mles; k++) {  // (a products handle: an unused MLE has no tables at all)
        // round 1 reads the input; round 2 folds input -> buf[0]; round j >= 3 folds buf[j & 1] ... alternating
        if (round == 1) a.src[k] = s->input[k];
        else if (round == 2) { a.src[k] = s->input[k]; a.dst[k] = s->buf[0][k]; }
        else { a.src[k] = s->buf[(round - 3) & 1][k]; a.dst[k] = s->buf[(round - 2) & 1][k]; }
    }
    if (a.fold)
        for (int i = 0; i < FL; i++) a.r[i] = r_prev[i];
}

template <int FL>
int32_t sumcheck_round_fl(zip_sumcheck *s, const uint64_t *r_prev) {
    SumcheckRoundArgs<FL> a{};
    sumcheck_fill_round<FL>(s, r_prev, a);
    a.n_terms = s->n_terms;
    for (uint32_t t = 0; t < s->n_terms; t++) a.term_mask[t] = s->term_mask[t];
    for (int i = 0; i < FL; i++) a.one[i] = s->field.r[i];
    const FieldDev<FL> fd = to_dev<FL>(s->field);
    switch (s->n_mles) {
        case 1: return sumcheck_round_k<FL, 1>(s, a, fd);
        case 2: return sumcheck_round_k<FL, 2>(s, a, fd);
        case 3: return sumcheck_round_k<FL, 3>(s, a, fd);
        case 4: return sumcheck_round_k<FL, 4>(s, a, fd);
        case 5: return launch_sumcheck_wide<FL, 5>(s, a, fd);
        case 6: return launch_sumcheck_wide<FL, 6>(s, a, fd);
        case 7: return launch_sumcheck_wide<FL, 7>(s, a, fd);
        default: return launch_sumcheck_wide<FL, 8>(s, a, fd);
    }
}

// A zip_sumcheck_init_products handle: one sumcheck_round_products_kernel per round over all tables, eight lanes per
// hypercube point, 32 points per workgroup.
template <int FL>
int32_t sumcheck_round_products_fl(zip_sumcheck *s, const uint64_t *r_prev) {
    SumcheckProductsArgs<FL> a{};
    sumcheck_fill_round<FL>(s, r_prev, a);
    a.n_products = s->n_terms;
    for (uint32_t t = 0; t < s->n_terms; t++) {
        a.n_factors[t] = s->n_factors[t];
        a.factors[t] = s->factors[t];
        a.own[t] = s->own[t];
        // (a single factor has no running term to negate or to start from: its coefficient is a multiplicand)
        if (s->n_factors[t] < 2) a.coeff_kind[t] = 0u;
    }
    auto kern = sumcheck_round_products_kernel<FL>;
    return launch_sumcheck_kernel<FL>(s, kern, "sumcheck_round_products_kernel", (size_t)256 * FL * 8, 256 / kSumcheckWideLanes, a,
                                      to_dev<FL>(s->field));
}

// ---- zip_sumcheck_prove: the transcript of MLSumcheck::prove_as_subprotocol inside the library ---------------------------
// Messages, challenges and the sponge of at most kTailMaxLog tail rounds
constexpr size_t kTailOutBytes = ((size_t)kTailMaxLog * (kSumcheckMaxDegree + 2) * 4 + 25 + kKeccakRateWords + 1) * 8;

// Process-wide launch counts of the sumcheck prover (zip_sumcheck_launch_counts: tests and tools tell from them which
// path a call took -- every path gives the same bytes)
std::atomic<uint64_t> g_sumcheck_round_launches{0}, g_sumcheck_tail_launches{0};

// the largest n for which K tables of 2^n entries and the kernel's static LDS fit one workgroup
uint32_t tail_lds_bound(uint32_t n_mles, uint32_t fl) {
    uint32_t n = 0;
    while (n < kTailMaxLog && ((size_t)n_mles << (n + 1)) * fl * 8 + kTailFixedLds <= kTailLdsTotal) n++;
    return n;
}

template <int FL>
int32_t sumcheck_prove_fl(zip_sumcheck *s, zip_keccak_state *transcript, uint64_t *msgs_out, uint64_t *randomness_out) {
    zip_ctx *ctx = s->ctx;
    const HostField &hf = s->field;
    const uint32_t nv = s->num_vars, ne = s->degree + 1;
    // (the sponge on this thread: TrSponge, keccak_dev.cuh -- the serial form of what the tail kernel does)
    TrSponge sp;
    memcpy(sp.st, transcript->st, sizeof sp.st);
    {
        uint8_t pending[kKeccakRate] = {0};
        memcpy(pending, transcript->buf, transcript->buflen);
        memcpy(sp.blk, pending, kKeccakRate);  // little-endian host
    }
    sp.buflen = transcript->buflen;
    const TrField<FL> tf = tr_make_field<FL>(hf.modulus, hf.r2, hf.inv);
    uint64_t v[2][FL];
    tr_map_u128<FL>(tf, nv, 0, v[0]);  // sumcheck.rs:64-76
    tr_map_u128<FL>(tf, s->degree, 0, v[1]);
    tr_sponge_absorb_fields<FL>(sp, tf, &v[0][0], 2);
    // The tail plays the last n rounds (tables of 2^n entries in its first).  ZIP_HIP_SUMCHECK_TAIL=n: 0 = no tail
    // kernel; more than fits the LDS for this shape: as much as fits.  (Per call: the tests flip it.)
    const uint32_t bound = tail_lds_bound(s->n_mles, FL);
    const uint32_t knob = (uint32_t)env_long("ZIP_HIP_SUMCHECK_TAIL", bound, 0, kTailMaxLog);
    // (a zip_sumcheck_init_products handle: sumcheck_tail_kernel does not know its combination function -- every round
    // goes through the round kernel and the sponge stays on this thread)
    const uint32_t n_tail = s->products ? 0u : std::min(std::min(knob, bound), nv);
    uint64_t r[FL] = {};
    for (uint32_t round = 0; round < nv - n_tail; round++) {  // the kernels and launch logic of zip_sumcheck_round
        uint64_t *msg = msgs_out + (size_t)round * ne * FL;
        if (int32_t rc = zip_sumcheck_round_begin(s, round ? r : nullptr)) return rc;
        if (int32_t rc = zip_sumcheck_round_end(s, msg)) return rc;
        tr_sponge_round<FL>(sp, tf, msg, ne, r);  // absorb_slice, get_challenge, absorb the challenge (sumcheck.rs:100-103)
        memcpy(randomness_out + (size_t)round * FL, r, 8 * FL);
    }
    if (n_tail) {
        SumcheckTailArgs<FL> a{};
        const uint32_t first = nv - n_tail + 1;  // 1-based round
        a.n_mles = s->n_mles;
        a.degree = s->degree;
        a.fold_first = first > 1;
        a.log_len = n_tail;
        a.n_terms = s->n_terms;
        for (uint32_t t = 0; t < s->n_terms; t++) {
            a.term_mask[t] = s->term_mask[t];
            for (int i = 0; i < FL; i++) a.coeff[t][i] = s->coeff[t][i];
        }
        for (uint32_t k = 0; k < s->n_mles; k++)  // what round `first` of zip_sumcheck_round would read
            a.src[k] = first <= 2 ? s->input[k] : s->buf[(first - 3) & 1][k];
        for (int i = 0; i < FL; i++) a.r[i] = r[i];
        memcpy(a.st, sp.st, sizeof a.st);
        memcpy(a.blk, sp.blk, sizeof a.blk);
        a.buflen = sp.buflen;
        a.tf = tf;
        a.out = s->tail_out_d;
        const size_t lds = ((size_t)s->n_mles << n_tail) * FL * 8;
        auto kern = sumcheck_tail_kernel<FL>;
        if (int32_t rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), lds)) return rc;
        {
            LaunchTimer t(ctx, "sumcheck_tail_kernel");
            hipLaunchKernelGGL(kern, dim3(1), dim3(kTailThreads), lds, ctx->stream, a, to_dev<FL>(hf));
            HIP_TRY(ctx, hipGetLastError());
            g_sumcheck_tail_launches++;
        }
        const size_t n_msg = (size_t)n_tail * ne * FL, n_ch = (size_t)n_tail * FL, n_words = n_msg + n_ch + 25 + kKeccakRateWords + 1;
        uint64_t host[kTailOutBytes / 8];
        HIP_TRY(ctx, hipMemcpyAsync(host, s->tail_out_d, n_words * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, stream_wait(ctx->stream));
        memcpy(msgs_out + (size_t)(nv - n_tail) * ne * FL, host, n_msg * 8);
        memcpy(randomness_out + (size_t)(nv - n_tail) * FL, host + n_msg, n_ch * 8);
        const uint64_t *so = host + n_msg + n_ch;
        memcpy(sp.st, so, sizeof sp.st);
        memcpy(sp.blk, so + 25, sizeof sp.blk);
        sp.buflen = (uint32_t)so[25 + kKeccakRateWords];
        s->round = nv;
    }
    memcpy(transcript->st, sp.st, sizeof sp.st);
    memcpy(transcript->buf, sp.blk, sizeof transcript->buf);  // zero beyond buflen
    transcript->buflen = sp.buflen;
    return ZIP_OK;
}

// ---- zip_sumcheck_prove_batch: n_instances sumchecks of one shape, one workgroup each, in ONE launch ---------------------
// Process-wide (zip_sumcheck_batch_counts): launches of sumcheck_batch_kernel, the instances they played and the rounds
// they played from HBM (max(0, num_vars - n) per instance, computed here at launch)
std::atomic<uint64_t> g_sumcheck_batch_launches{0}, g_sumcheck_batch_instances{0}, g_sumcheck_batch_streamed{0};
// HOST tables up to this size are gathered into the pinned bounce pair instead of being copied one by one (a copy
// call costs ~10 us: as much as 256 KiB take through a memcpy)
constexpr size_t kBatchPackBytes = (size_t)256 << 10;

// The arguments have been checked and fields[i] made; `ctx` is the call's own plumbing context (its blocks come from
// the recycle bin and go back there).  Transcripts are written only after everything has succeeded.
template <int FL>
int32_t sumcheck_prove_batch_fl(zip_ctx *ctx, const zip_sumcheck_instance *inst, uint32_t B, zip_mem_kind kind, uint32_t n_mles,
                                uint32_t nv, uint32_t degree, const std::vector<HostField> &fields, uint64_t *msgs_out,
                                uint64_t *randomness_out) {
    const uint32_t ne = degree + 1;
    // The last n rounds are played from LDS.  ZIP_HIP_SUMCHECK_TAIL=n as for zip_sumcheck_prove (per call: the tests flip
    // it); here 0 means that every round is streamed.  The kernel's static LDS is the tail kernel's: the same bound.
    const uint32_t bound = tail_lds_bound(n_mles, FL);
    const uint32_t knob = (uint32_t)env_long("ZIP_HIP_SUMCHECK_TAIL", bound, 0, kTailMaxLog);
    const uint32_t n_lds = std::min(std::min(knob, bound), nv), n_streamed = nv - n_lds;
    const size_t elem = (size_t)FL * 8, tab_bytes = elem << nv, scr_bytes = n_streamed >= 2 ? (size_t)n_mles * (tab_bytes / 2) : 0;
    const size_t out_words = sumcheck_batch_out_words(nv, degree, FL);
    SumcheckBatchInst<FL> *args_d = nullptr;
    uint64_t *out_d = nullptr, *tables_d = nullptr, *scratch_d = nullptr;
    int32_t rc;
    if ((rc = pool_alloc(ctx, (size_t)B * sizeof(SumcheckBatchInst<FL>), (void **)&args_d))) return rc;
    if ((rc = pool_alloc(ctx, (size_t)B * out_words * 8, (void **)&out_d))) return rc;
    if (scr_bytes && (rc = pool_alloc(ctx, (size_t)B * scr_bytes, (void **)&scratch_d))) return rc;
    if (kind == ZIP_MEM_HOST) {
        const size_t n_tabs = (size_t)B * n_mles;
        if ((rc = pool_alloc(ctx, n_tabs * tab_bytes, (void **)&tables_d))) return rc;
        unsigned char *dst = reinterpret_cast<unsigned char *>(tables_d);
        if (tab_bytes <= kBatchPackBytes && n_tabs > 1) {
            // small tables: a copy call apiece costs more than the bytes do -- gathered into the pinned bounce pair, one
            // copy per buffer-full, the gather of the next beside the copy of this one
            if ((rc = ensure_bounce(ctx, kBounceBytes))) return rc;
            const size_t per = ctx->bounce_cap / tab_bytes;  // tables per buffer-full
            hipEvent_t ev[2] = {take_dep_event(ctx), take_dep_event(ctx)};
            size_t chunk = 0;
            for (size_t at = 0; at < n_tabs && rc == ZIP_OK; at += per, chunk++) {
                const size_t n = std::min(per, n_tabs - at);
                unsigned char *b = ctx->bounce[chunk & 1];
                if (chunk >= 2 && event_wait(ev[chunk & 1]) != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "host-to-device copy failed"); break; }
                for (size_t t = 0; t < n; t++) memcpy(b + t * tab_bytes, inst[(at + t) / n_mles].mles[(at + t) % n_mles], tab_bytes);
                hipError_t e = hipMemcpyAsync(dst + at * tab_bytes, b, n * tab_bytes, hipMemcpyHostToDevice, ctx->stream);
                if (e == hipSuccess) e = hipEventRecord(ev[chunk & 1], ctx->stream);
                if (e != hipSuccess) rc = fail(ctx, ZIP_ERR_HIP, "host-to-device copy failed: %s", hipGetErrorString(e));
            }
            ctx->dep_event_pool.push_back(ev[0]);
            ctx->dep_event_pool.push_back(ev[1]);
            if (rc) return rc;  // (the context's destruction waits for the stream before the pair is handed on)
        } else {
            for (size_t t = 0; t < n_tabs; t++)
                if ((rc = copy_h2d_bounced(ctx, dst + t * tab_bytes, inst[t / n_mles].mles[t % n_mles], tab_bytes, ctx->stream))) return rc;
        }
    }
    std::vector<SumcheckBatchInst<FL>> args(B);
    for (uint32_t i = 0; i < B; i++) {
        SumcheckBatchInst<FL> &a = args[i];
        memset(&a, 0, sizeof a);
        const HostField &hf = fields[i];
        for (uint32_t k = 0; k < n_mles; k++)
            a.src[k] = kind == ZIP_MEM_HOST ? tables_d + (((size_t)i * n_mles + k) << nv) * FL : inst[i].mles[k];
        a.scratch = scr_bytes ? scratch_d + (size_t)i * (scr_bytes / 8) : nullptr;
        a.f = to_dev<FL>(hf);
        a.tf = tr_make_field<FL>(hf.modulus, hf.r2, hf.inv);
        if (const zip_sumcheck_comb *c = inst[i].comb) {
            a.n_terms = c->n_terms;
            for (uint32_t t = 0; t < c->n_terms; t++) {
                a.term_mask[t] = c->term_mask[t];
                for (int l = 0; l < FL; l++) a.coeff[t][l] = c->coeff[t][l];
            }
        }
        const zip_keccak_state *tr = inst[i].transcript;
        memcpy(a.st, tr->st, sizeof a.st);
        memcpy(a.blk, tr->buf, tr->buflen);  // little-endian host; zero beyond buflen
        a.buflen = tr->buflen;
        a.out = out_d + (size_t)i * out_words;
    }
    HIP_TRY(ctx, hipMemcpyAsync(args_d, args.data(), (size_t)B * sizeof(SumcheckBatchInst<FL>), hipMemcpyHostToDevice, ctx->stream));
    const size_t lds = n_lds ? ((size_t)n_mles << n_lds) * elem : 0;
    auto kern = sumcheck_batch_kernel<FL>;
    if ((rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void *>(kern), lds))) return rc;
    {
        LaunchTimer t(ctx, "sumcheck_batch_kernel");
        hipLaunchKernelGGL(kern, dim3(B), dim3(kTailThreads), lds, ctx->stream, (const SumcheckBatchInst<FL> *)args_d, n_mles, degree, nv, n_lds);
        HIP_TRY(ctx, hipGetLastError());
        g_sumcheck_batch_launches++;
        g_sumcheck_batch_instances += B;
        g_sumcheck_batch_streamed += (uint64_t)B * n_streamed;
    }
    std::vector<uint64_t> host((size_t)B * out_words);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), out_d, host.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    const size_t n_msg = (size_t)nv * ne * FL, n_ch = (size_t)nv * FL;
    for (uint32_t i = 0; i < B; i++) {
        const uint64_t *o = host.data() + (size_t)i * out_words, *so = o + n_msg + n_ch;
        memcpy(msgs_out + (size_t)i * n_msg, o, n_msg * 8);
        memcpy(randomness_out + (size_t)i * n_ch, o + n_msg, n_ch * 8);
        zip_keccak_state *tr = inst[i].transcript;
        memcpy(tr->st, so, sizeof tr->st);
        memcpy(tr->buf, so + 25, sizeof tr->buf);  // zero beyond buflen
        tr->buflen = (uint32_t)so[25 + kKeccakRateWords];
    }
    return ZIP_OK;
}

// ---- zip_get_prime / zip_prime_test_base2: prime_gen::get_prime (src/prime_gen.rs:15-28) -------------------------------
// The candidate chain (prime_next_candidate, prime_dev.cuh) does not depend on any verdict, so this thread hashes a
// batch ahead, hands it to prime_test_base2_kernel -- one candidate per lane -- and hashes the next batch while that one
// is on the device.  Per candidate it keeps the sponge as the reference's loop holds it when it tests that candidate:
// the call ends with the winner's, and nothing of the candidates speculated beyond it is left.
// Per device, made at the first call and kept: a stream, and two slots (the batch in flight and the batch being hashed)
// of pinned host and of device memory, each [kPrimeMaxBatch candidates of 4 limbs | kPrimeMaxBatch verdict bytes].
constexpr uint32_t kPrimeMaxBatch = 4096, kPrimeMaxCandidates = 65536;
// (the default width: the lowest SUM of the three per-limb-count medians of the zip_get_prime time over the twelve
// transcripts of profiles/prime_gen.md -- 64 has the lower median at 2 and 3 limbs, 128 at 4 limbs and on the sum)
constexpr uint32_t kPrimeDefaultBatch = 128;
constexpr size_t kPrimeVerdictsAt = (size_t)kPrimeMaxBatch * 4 * 8, kPrimeSlotBytes = kPrimeVerdictsAt + kPrimeMaxBatch;
struct PrimeDev {
    std::mutex mu;  // one call at a time per device
    hipStream_t stream = nullptr;
    unsigned char *host = nullptr, *dev = nullptr;
    unsigned char *batch_dev = nullptr;  // zip_get_prime_batch: grown to the largest call so far, up to kPrimeBatchKeepBytes
    size_t batch_bytes = 0;
};
PrimeDev g_prime[kMaxDevices];
// Process-wide (zip_prime_launch_counts): launches of prime_test_base2_kernel and the candidates they tested
std::atomic<uint64_t> g_prime_launches{0}, g_prime_candidates{0};

// zip_prime_test_base2 / zip_get_prime take a device ordinal, not a ctx: the calling thread's current device is put
// back when they return
struct CurrentDeviceGuard {
    int prev = -1;
    CurrentDeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~CurrentDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// a failed enqueue or wait: nothing of this call may still be queued on the slots the next call reuses
int32_t prime_fail_drained(PrimeDev &pd) {
    (void)hipStreamSynchronize(pd.stream);
    return ZIP_ERR_HIP;
}

int32_t prime_dev_ready(PrimeDev &pd, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || device >= kMaxDevices) return ZIP_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return ZIP_ERR_NO_DEVICE;
    if (!pd.stream && hipStreamCreateWithFlags(&pd.stream, hipStreamNonBlocking) != hipSuccess) {
        pd.stream = nullptr;
        return ZIP_ERR_HIP;
    }
    if (!pd.host && hipHostMalloc((void **)&pd.host, 2 * kPrimeSlotBytes, hipHostMallocDefault) != hipSuccess) {
        pd.host = nullptr;
        return ZIP_ERR_ALLOC;
    }
    if (!pd.dev && hipMalloc((void **)&pd.dev, 2 * kPrimeSlotBytes) != hipSuccess) {
        pd.dev = nullptr;
        return ZIP_ERR_ALLOC;
    }
    return ZIP_OK;
}
void prime_dev_release(int device) {  // (the device is current)
    PrimeDev &pd = g_prime[device];
    std::lock_guard<std::mutex> g(pd.mu);
    if (pd.stream) (void)hipStreamSynchronize(pd.stream);
    if (pd.dev) (void)hipFree(pd.dev);
    if (pd.batch_dev) (void)hipFree(pd.batch_dev);
    if (pd.host) (void)hipHostFree(pd.host);
    if (pd.stream) (void)hipStreamDestroy(pd.stream);
    pd.dev = pd.host = pd.batch_dev = nullptr;
    pd.batch_bytes = 0;
    pd.stream = nullptr;
}

// the n <= kPrimeMaxBatch candidates in the host half of `slot`: up, one launch, the verdicts down -- enqueued, not waited for
template <int FL>
hipError_t prime_enqueue(PrimeDev &pd, uint32_t slot, uint32_t n) {
    unsigned char *h = pd.host + slot * kPrimeSlotBytes, *d = pd.dev + slot * kPrimeSlotBytes;
    hipError_t e = hipMemcpyAsync(d, h, (size_t)n * FL * 8, hipMemcpyHostToDevice, pd.stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(prime_test_base2_kernel<FL>, dim3((n + kPrimeThreads - 1) / kPrimeThreads), dim3(kPrimeThreads), 0,
                       pd.stream, reinterpret_cast<const uint64_t *>(d), n, d + kPrimeVerdictsAt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    g_prime_launches++;
    g_prime_candidates += n;
    return hipMemcpyAsync(h + kPrimeVerdictsAt, d + kPrimeVerdictsAt, n, hipMemcpyDeviceToHost, pd.stream);
}

template <int FL>
int32_t prime_test_fl(PrimeDev &pd, const uint64_t *candidates, uint32_t n, uint8_t *verdicts_out) {
    for (uint32_t at = 0; at < n; at += kPrimeMaxBatch) {
        const uint32_t take = std::min(n - at, kPrimeMaxBatch);
        memcpy(pd.host, candidates + (size_t)at * FL, (size_t)take * FL * 8);
        if (prime_enqueue<FL>(pd, 0, take) != hipSuccess || stream_wait(pd.stream) != hipSuccess) return prime_fail_drained(pd);
        memcpy(verdicts_out + at, pd.host + kPrimeVerdictsAt, take);
    }
    return ZIP_OK;
}

template <int FL>
int32_t get_prime_fl(PrimeDev &pd, zip_keccak_state *transcript, uint32_t batch, uint64_t *prime_out, uint32_t *tried_out) {
    TrSponge sp;
    memcpy(sp.st, transcript->st, sizeof sp.st);
    {
        uint8_t pending[kKeccakRate] = {0};
        memcpy(pending, transcript->buf, transcript->buflen);
        memcpy(sp.blk, pending, kKeccakRate);  // little-endian host
    }
    sp.buflen = transcript->buflen;
    std::vector<TrSponge> after[2];  // after[slot][k]: the sponge once candidate k of that slot's batch is absorbed
    after[0].resize(batch);
    after[1].resize(batch);
    auto hash = [&](uint32_t slot, uint32_t from, uint32_t to) {  // candidates [from, to) of the batch in `slot`
        uint64_t *c = reinterpret_cast<uint64_t *>(pd.host + slot * kPrimeSlotBytes);
        for (uint32_t k = from; k < to; k++) {
            uint64_t cand[FL];
            prime_next_candidate<FL>(sp, cand);
            memcpy(c + (size_t)k * FL, cand, sizeof cand);
            after[slot][k] = sp;
        }
    };
    for (uint32_t done = 0, slot = 0, ahead = 0; done < kPrimeMaxCandidates; done += batch, slot ^= 1) {
        hash(slot, ahead, batch);  // (the first batch; later, what the previous round left of this one)
        const uint32_t n = std::min(batch, kPrimeMaxCandidates - done);
        if (prime_enqueue<FL>(pd, slot, n) != hipSuccess) return prime_fail_drained(pd);
        // the next batch's chain while this one is on the device -- eight candidates between two looks at the stream,
        // and no further once the verdicts are in: a winner among them ends the call without the rest of the hashing
        hipError_t q = hipErrorNotReady;
        for (ahead = 0; ahead < batch && q == hipErrorNotReady; ahead = std::min(ahead + 8, batch)) {
            hash(slot ^ 1, ahead, std::min(ahead + 8, batch));
            q = hipStreamQuery(pd.stream);
        }
        clear_not_ready();
        if (q == hipErrorNotReady) q = stream_wait(pd.stream);
        if (q != hipSuccess) return prime_fail_drained(pd);
        const unsigned char *h = pd.host + slot * kPrimeSlotBytes;
        for (uint32_t k = 0; k < n; k++) {
            if (!h[kPrimeVerdictsAt + k]) continue;
            memcpy(prime_out, h + (size_t)k * FL * 8, (size_t)FL * 8);
            if (tried_out) *tried_out = done + k + 1;
            const TrSponge &w = after[slot][k];
            memcpy(transcript->st, w.st, sizeof w.st);
            memcpy(transcript->buf, w.blk, sizeof transcript->buf);  // zero beyond buflen
            transcript->buflen = w.buflen;
            return ZIP_OK;
        }
    }
    fprintf(stderr, "zip_get_prime: no probable prime among the first %u candidates of %d limbs; giving up\n",
            kPrimeMaxCandidates, FL);
    return ZIP_ERR_UNSUPPORTED;
}

// ---- zip_get_prime_batch: get_prime on n independent transcripts, the candidate chains on the device ---------------------
// (kernels_prime_batch.cuh.)  A round is w candidates per live member and four launches: chain, test, reduce, replay;
// then the number of members still live comes back -- the one host synchronisation of the round.  The launches of a call
// therefore follow the rounds of its longest chain, not n.  One copy of the sponges up, one copy of [winners' sponges |
// primes | positions] back.  One device block per call: [A | B | result | candidates | live lists, steps, counts |
// verdicts]; a block of up to kPrimeBatchKeepBytes stays with the device for the next call, a larger one is freed.
constexpr uint32_t kPrimeBatchDefaultWindow = 64, kPrimeBatchMaxWindow = 1024, kPrimeBatchMaxMembers = 65535;
constexpr size_t kPrimeBatchKeepBytes = (size_t)64 << 20;
// Process-wide (zip_prime_batch_counts): successful calls, their members, and the kernel launches they made
std::atomic<uint64_t> g_prime_batch_calls{0}, g_prime_batch_members{0}, g_prime_batch_launches{0};

template <int FL>
int32_t get_prime_batch_fl(PrimeDev &pd, zip_keccak_state *transcripts, uint32_t n, uint32_t w, uint64_t *primes_out,
                           uint32_t *tried_out) {
    const size_t N = n, sponge_words = (size_t)kPrimeSpongeWords * N;
    // (every piece a multiple of 8 bytes)
    const size_t result_words = sponge_words + N * FL + (N + 1) / 2;
    const size_t cand_words = N * w * FL, list_words = (N + 1) / 2;
    const size_t at_b = sponge_words, at_result = 2 * sponge_words, at_cands = at_result + result_words,
                 at_live0 = at_cands + cand_words, at_live1 = at_live0 + list_words, at_steps = at_live1 + list_words,
                 at_counts = at_steps + list_words, at_verdicts = at_counts + 1;
    const size_t bytes = at_verdicts * 8 + N * w;
    unsigned char *block = pd.batch_dev;
    const bool own = bytes > pd.batch_bytes && bytes > kPrimeBatchKeepBytes;  // too large to keep: this call's alone
    if (bytes > pd.batch_bytes) {
        if (hipMalloc((void **)&block, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return ZIP_ERR_ALLOC;
        }
        if (!own) {
            if (pd.batch_dev) (void)hipFree(pd.batch_dev);
            pd.batch_dev = block;
            pd.batch_bytes = bytes;
        }
    }
    struct Release {
        unsigned char *p;
        ~Release() { if (p) (void)hipFree(p); }
    } release{own ? block : nullptr};
    uint64_t *base = reinterpret_cast<uint64_t *>(block);
    uint64_t *sp_a = base, *sp_b = base + at_b, *result = base + at_result, *cands = base + at_cands;
    uint64_t *primes_d = result + sponge_words;
    uint32_t *tried_d = reinterpret_cast<uint32_t *>(primes_d + N * FL);
    uint32_t *lists[2] = {reinterpret_cast<uint32_t *>(base + at_live0), reinterpret_cast<uint32_t *>(base + at_live1)};
    uint32_t *steps = reinterpret_cast<uint32_t *>(base + at_steps), *counts = reinterpret_cast<uint32_t *>(base + at_counts);
    uint8_t *verdicts = block + at_verdicts * 8;

    std::vector<uint64_t> up(sponge_words), down(result_words);
    for (size_t m = 0; m < N; m++) {
        const zip_keccak_state &t = transcripts[m];
        uint64_t blk[kKeccakRateWords] = {0};
        memcpy(blk, t.buf, t.buflen);  // little-endian host; zero beyond buflen
        for (uint32_t i = 0; i < 25; i++) up[(size_t)i * N + m] = t.st[i];
        for (uint32_t i = 0; i < kKeccakRateWords; i++) up[(size_t)(25 + i) * N + m] = blk[i];
        up[(size_t)(kPrimeSpongeWords - 1) * N + m] = t.buflen;
    }
    if (hipMemcpyAsync(sp_a, up.data(), sponge_words * 8, hipMemcpyHostToDevice, pd.stream) != hipSuccess)
        return prime_fail_drained(pd);

    uint32_t *n_live_h = reinterpret_cast<uint32_t *>(pd.host);  // pinned; the slots of zip_get_prime are idle under pd.mu
    uint64_t launches = 0;
    uint32_t n_live = n, done = 0;
    const uint32_t *live = nullptr;  // round 0: member j is lane j
    for (uint32_t round = 0; n_live && done < kPrimeMaxCandidates; round++) {
        const uint32_t wr = std::min(w, kPrimeMaxCandidates - done);
        uint32_t *live_next = lists[round & 1], *n_next = counts + (round & 1);
        const dim3 members((n_live + kPrimeThreads - 1) / kPrimeThreads), wave(kPrimeThreads);
        const uint32_t n_cands = n_live * wr;  // <= 65535 * 1024
        if (hipMemsetAsync(n_next, 0, sizeof(uint32_t), pd.stream) != hipSuccess) return prime_fail_drained(pd);
        hipLaunchKernelGGL(prime_chain_batch_kernel<FL>, members, wave, 0, pd.stream, (const uint64_t *)sp_a, sp_b, n, live, n_live,
                           (const uint32_t *)nullptr, wr, cands);
        hipLaunchKernelGGL(prime_test_base2_kernel<FL>, dim3((n_cands + kPrimeThreads - 1) / kPrimeThreads), wave, 0, pd.stream,
                           (const uint64_t *)cands, n_cands, verdicts);
        hipLaunchKernelGGL(prime_reduce_batch_kernel<FL>, members, wave, 0, pd.stream, (const uint64_t *)cands,
                           (const uint8_t *)verdicts, n, live, n_live, wr, done, primes_d, tried_d, steps, live_next, n_next);
        hipLaunchKernelGGL(prime_chain_batch_kernel<FL>, members, wave, 0, pd.stream, (const uint64_t *)sp_a, result, n, live, n_live,
                           (const uint32_t *)steps, wr, (uint64_t *)nullptr);
        if (hipGetLastError() != hipSuccess) return prime_fail_drained(pd);
        launches += 4;
        if (hipMemcpyAsync(n_live_h, n_next, sizeof(uint32_t), hipMemcpyDeviceToHost, pd.stream) != hipSuccess ||
            stream_wait(pd.stream) != hipSuccess)
            return prime_fail_drained(pd);
        n_live = std::min(*n_live_h, n_live);
        live = live_next;
        std::swap(sp_a, sp_b);  // the members still live go on from where this round's chain ended
        done += wr;
    }
    if (n_live) {
        fprintf(stderr, "zip_get_prime_batch: %u of %u members have no probable prime among their first %u candidates of %d limbs; giving up\n",
                n_live, n, kPrimeMaxCandidates, FL);
        return ZIP_ERR_UNSUPPORTED;
    }
    if (hipMemcpyAsync(down.data(), result, result_words * 8, hipMemcpyDeviceToHost, pd.stream) != hipSuccess ||
        stream_wait(pd.stream) != hipSuccess)
        return prime_fail_drained(pd);
    const uint32_t *tried_h = reinterpret_cast<const uint32_t *>(down.data() + sponge_words + N * FL);
    for (size_t m = 0; m < N; m++) {
        zip_keccak_state &t = transcripts[m];
        uint64_t blk[kKeccakRateWords];
        for (uint32_t i = 0; i < 25; i++) t.st[i] = down[(size_t)i * N + m];
        for (uint32_t i = 0; i < kKeccakRateWords; i++) blk[i] = down[(size_t)(25 + i) * N + m];
        memcpy(t.buf, blk, sizeof t.buf);  // zero beyond buflen
        t.buflen = (uint32_t)down[(size_t)(kPrimeSpongeWords - 1) * N + m];
        if (tried_out) tried_out[m] = tried_h[m];
    }
    memcpy(primes_out, down.data() + sponge_words, N * FL * 8);
    g_prime_batch_calls++;
    g_prime_batch_members += n;
    g_prime_batch_launches += launches;
    return ZIP_OK;
}

// ------------------------------------------------------------------ Spartan pieces
template <int FL>
int32_t ccs_map_i64(zip_ctx *ctx, const int64_t *in_d, uint64_t n_in, uint64_t n_out, uint64_t *out_d, const HostField &hf) {
    if (!n_out) return ZIP_OK;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_out + 255) / 256, 65535);
    LaunchTimer t(ctx, "field_map_i64_kernel");
    hipLaunchKernelGGL(field_map_i64_kernel<FL>, dim3(blocks), dim3(256), 0, ctx->stream, in_d, n_in, n_out, out_d,
                       to_dev<FL>(hf), hf.quirk_mod);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

template <int FL>
int32_t ccs_set_z_fl(zip_ccs *c, const int64_t *z_d, size_t z_len, const HostField &hf) {
    zip_ctx *ctx = c->ctx;
    int32_t rc;
    if ((rc = ccs_map_i64<FL>(ctx, z_d, z_len, c->m, c->z_f, hf))) return rc;
    const FieldDev<FL> fd = to_dev<FL>(hf);
    for (uint32_t k = 0; k < c->t; k++) {
        LaunchTimer t(ctx, "spmv_rows_kernel");
        hipLaunchKernelGGL(spmv_rows_kernel<FL>, dim3((c->m + 255) / 256), dim3(256), 0, ctx->stream, c->mat[k].row_ptr,
                           c->mat[k].col_idx, c->mat[k].vals, c->z_f, c->mat[k].n_rows, c->m, c->mz[k], fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    return ZIP_OK;
}

template <int FL>
int32_t ccs_eq_table_fl(zip_ccs *c, const uint64_t *r_d, uint32_t slot, const HostField &hf) {
    zip_ctx *ctx = c->ctx;
    const FieldDev<FL> fd = to_dev<FL>(hf);
    auto direct = [&](const uint64_t *r, uint32_t nv, uint64_t *out) -> int32_t {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((((uint64_t)1 << nv) + 255) / 256, 65535);
        LaunchTimer t(ctx, "eq_table_kernel");
        hipLaunchKernelGGL(eq_table_kernel<FL>, dim3(blocks), dim3(256), 0, ctx->stream, r, nv, out, fd);
        HIP_TRY(ctx, hipGetLastError());
        return ZIP_OK;
    };
    if (c->s < 12) return direct(r_d, c->s, c->eq[slot]);
    // eq(x, r) = eq(x_lo, r_lo) * eq(x_hi, r_hi): two small tables, then one multiplication per entry
    const uint32_t nv_lo = c->s / 2, nv_hi = c->s - nv_lo;
    uint64_t *lo = c->eq_half, *hi = c->eq_half + ((size_t)FL << nv_lo);
    int32_t rc;
    if ((rc = direct(r_d, nv_lo, lo))) return rc;
    if ((rc = direct(r_d + (size_t)nv_lo * FL, nv_hi, hi))) return rc;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)c->m + 255) / 256, 65535);
    LaunchTimer t(ctx, "eq_outer_kernel");
    hipLaunchKernelGGL(eq_outer_kernel<FL>, dim3(blocks), dim3(256), 0, ctx->stream, lo, hi, nv_lo, (uint64_t)c->m, c->eq[slot], fd);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

template <int FL>
int32_t ccs_second_fl(zip_ccs *c, const uint64_t *gamma_d, uint64_t *vs_d, const HostField &hf) {
    zip_ctx *ctx = c->ctx;
    const FieldDev<FL> fd = to_dev<FL>(hf);
    SecondTableArgs a{};
    for (uint32_t k = 0; k < c->t; k++) {
        a.col_ptr[k] = c->mat[k].col_ptr;
        a.row_idx[k] = c->mat[k].row_idx;
        a.vals[k] = c->mat[k].vals_t;
    }
    a.t = c->t;
    a.m = c->m;
    a.eq = c->eq[1];
    a.out = c->second;
    {
        LaunchTimer t(ctx, "second_table_kernel");
        hipLaunchKernelGGL(second_table_kernel<FL>, dim3((c->m + 255) / 256), dim3(256), 0, ctx->stream, a, gamma_d, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    for (uint32_t k = 0; k < c->t; k++) {  // calculate_V_s
        LaunchTimer t(ctx, "field_dot_partials_kernel");
        hipLaunchKernelGGL(field_dot_partials_kernel<FL>, dim3(c->dot_blocks), dim3(256), 0, ctx->stream, c->mz[k], c->eq[1],
                           (uint64_t)c->m, c->partials, fd);
        hipLaunchKernelGGL(sumcheck_reduce_kernel<FL>, dim3(1), dim3(256), 0, ctx->stream, c->partials, c->dot_blocks, 1u,
                           vs_d + (size_t)k * FL, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    return ZIP_OK;
}

template <int FL>
int32_t ccs_eval_matrices_fl(zip_ccs *c, uint64_t *out_d, const HostField &hf) {
    zip_ctx *ctx = c->ctx;
    const FieldDev<FL> fd = to_dev<FL>(hf);
    for (uint32_t k = 0; k < c->t; k++) {
        LaunchTimer t(ctx, "matrix_eval_partials_kernel");
        hipLaunchKernelGGL(matrix_eval_partials_kernel<FL>, dim3(c->dot_blocks), dim3(256), 0, ctx->stream, c->mat[k].row_ptr,
                           c->mat[k].col_idx, c->mat[k].vals, c->eq[0], c->eq[1], c->mat[k].n_rows, c->partials, fd);
        hipLaunchKernelGGL(sumcheck_reduce_kernel<FL>, dim3(1), dim3(256), 0, ctx->stream, c->partials, c->dot_blocks, 1u,
                           out_d + (size_t)k * FL, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    return ZIP_OK;
}

// ---- zip_ccs_batch: the same tables for n proofs of one circuit, launches per call independent of n ----------------------
// Process-wide (zip_ccs_batch_counts): kernel launches of the zip_ccs_batch_* calls and the instances handed to set_z
std::atomic<uint64_t> g_ccs_batch_launches{0}, g_ccs_batch_instances{0};

// table j of an instance: 0 z_f, 1 .. t M_k z, t + 1 / t + 2 eq slot 0 / 1, t + 3 the second sumcheck's table
uint64_t *ccs_batch_table_at(const zip_ccs_batch *b, uint32_t instance, uint32_t j) {
    return b->tables + ((((size_t)instance * (b->t + 4) + j) << b->s) * b->fl);
}

// waits for everything enqueued so far; the host staging vectors are free afterwards
int32_t ccs_batch_wait(zip_ccs_batch *b) {
    if (!b->in_flight) return ZIP_OK;
    HIP_TRY(b->ctx, stream_wait(b->ctx->stream));
    b->in_flight = false;
    return ZIP_OK;
}

// the per-instance argument array into b->args_h; z_dev[i]: where instance i's z lies on the device
template <int FL>
void ccs_batch_fill_args(zip_ccs_batch *b, const std::vector<HostField> &fields, const std::vector<const int64_t *> &z_dev,
                         const size_t *z_len, uint32_t n) {
    b->args_h.assign((size_t)n * sizeof(CcsBatchInst<FL>), 0);
    CcsBatchInst<FL> *args = reinterpret_cast<CcsBatchInst<FL> *>(b->args_h.data());
    for (uint32_t i = 0; i < n; i++) {
        CcsBatchInst<FL> &a = args[i];
        a.f = to_dev<FL>(fields[i]);
        a.quirk_mod = fields[i].quirk_mod;
        a.z = z_dev[i];
        a.z_len = z_len[i];
        a.z_f = ccs_batch_table_at(b, i, 0);
        for (uint32_t k = 0; k < b->t; k++) a.mz[k] = ccs_batch_table_at(b, i, 1 + k);
        a.eq[0] = ccs_batch_table_at(b, i, b->t + 1);
        a.eq[1] = ccs_batch_table_at(b, i, b->t + 2);
        a.second = ccs_batch_table_at(b, i, b->t + 3);
    }
}

template <int FL>
int32_t ccs_batch_set_z_fl(zip_ccs_batch *b) {
    zip_ctx *ctx = b->ctx;
    const CcsBatchInst<FL> *args = static_cast<const CcsBatchInst<FL> *>(b->args_d);
    const uint32_t bx = (b->m + 255) / 256;
    {
        LaunchTimer t(ctx, "ccs_batch_map_z_kernel");
        hipLaunchKernelGGL(ccs_batch_map_z_kernel<FL>, dim3(bx, b->n), dim3(256), 0, ctx->stream, args, b->m);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        LaunchTimer t(ctx, "ccs_batch_spmv_kernel");
        hipLaunchKernelGGL(ccs_batch_spmv_kernel<FL>, dim3(bx, b->t, b->n), dim3(256), 0, ctx->stream, b->mats, args);
        HIP_TRY(ctx, hipGetLastError());
    }
    g_ccs_batch_launches += 2;
    return ZIP_OK;
}

// eq(x, r_i) for every instance into `slot`; r_d: n * s elements on the device
template <int FL>
int32_t ccs_batch_eq_fl(zip_ccs_batch *b, const uint64_t *r_d, uint32_t slot) {
    zip_ctx *ctx = b->ctx;
    LaunchTimer t(ctx, "ccs_batch_eq_kernel");
    hipLaunchKernelGGL(ccs_batch_eq_kernel<FL>, dim3((b->m + kCcsBatchEqPerBlock - 1) / kCcsBatchEqPerBlock, b->n), dim3(256), 0,
                       ctx->stream, static_cast<const CcsBatchInst<FL> *>(b->args_d), r_d, b->s, slot);
    HIP_TRY(ctx, hipGetLastError());
    g_ccs_batch_launches++;
    return ZIP_OK;
}

template <int FL>
int32_t ccs_batch_second_fl(zip_ccs_batch *b, const uint64_t *gamma_d) {
    zip_ctx *ctx = b->ctx;
    const CcsBatchInst<FL> *args = static_cast<const CcsBatchInst<FL> *>(b->args_d);
    {
        LaunchTimer t(ctx, "ccs_batch_second_kernel");
        hipLaunchKernelGGL(ccs_batch_second_kernel<FL>, dim3((b->m + 255) / 256, b->n), dim3(256), 0, ctx->stream, b->mats, args, gamma_d);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        LaunchTimer t(ctx, "ccs_batch_vs_kernel");  // calculate_V_s
        hipLaunchKernelGGL(ccs_batch_vs_kernel<FL>, dim3(b->t, b->n), dim3(kCcsBatchVsThreads), 0, ctx->stream, args, b->m, b->vs_d);
        HIP_TRY(ctx, hipGetLastError());
    }
    g_ccs_batch_launches += 2;
    return ZIP_OK;
}

// V_xy of every instance from eq slot 0 (r_x) and slot 1 (r_y) into vs_d
template <int FL>
int32_t ccs_batch_eval_matrices_fl(zip_ccs_batch *b) {
    zip_ctx *ctx = b->ctx;
    LaunchTimer t(ctx, "ccs_batch_eval_matrices_kernel");
    hipLaunchKernelGGL(ccs_batch_eval_matrices_kernel<FL>, dim3(b->t, b->n), dim3(kCcsBatchVsThreads), 0, ctx->stream, b->mats,
                       static_cast<const CcsBatchInst<FL> *>(b->args_d), b->vs_d);
    HIP_TRY(ctx, hipGetLastError());
    g_ccs_batch_launches++;
    return ZIP_OK;
}
}  // namespace

// =============================================================================
// exported symbols
// =============================================================================
// ------------------------------------------------------------------ batches (kernels_batch.cuh)
namespace {
template <int FL>
int32_t launch_batch_combine_fl(zip_ctx *ctx, BatchCombineArgs a, uint32_t n_polys, bool do_int, const HostField &hf) {
    const FieldDev<FL> fd = to_dev<FL>(hf);
    const dim3 grid((a.row_len + kBatchCombineThreads - 1) / kBatchCombineThreads, n_polys), block(kBatchCombineThreads);
    LaunchTimer t(ctx, "batch_combine_kernel", ctx->stream);
    if (a.quirk_mod) {  // (rare moduli: the instances that carry the 64-bit division)
        if (do_int) hipLaunchKernelGGL((batch_combine_kernel<FL, true, true>), grid, block, 0, ctx->stream, a, fd);
        else hipLaunchKernelGGL((batch_combine_kernel<FL, false, true>), grid, block, 0, ctx->stream, a, fd);
    } else {
        if (do_int) hipLaunchKernelGGL((batch_combine_kernel<FL, true, false>), grid, block, 0, ctx->stream, a, fd);
        else hipLaunchKernelGGL((batch_combine_kernel<FL, false, false>), grid, block, 0, ctx->stream, a, fd);
    }
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}
int32_t launch_batch_combine(zip_ctx *ctx, const BatchCombineArgs &a, uint32_t n_polys, bool do_int, const HostField &hf) {
    return with_fl(hf.fl, [&](auto FL) { return launch_batch_combine_fl<decltype(FL)::value>(ctx, a, n_polys, do_int, hf); });
}

// BatchFieldInst<FL>[B] for batch_combine_fields_kernel, and the members' 1_mont (what a one-row batch multiplies by)
template <int FL>
void batch_fill_field_args(const std::vector<HostField> &hf, std::vector<unsigned char> *inst, std::vector<uint64_t> *ones) {
    inst->assign(hf.size() * sizeof(BatchFieldInst<FL>), 0);
    ones->resize(hf.size() * FL);
    BatchFieldInst<FL> *a = reinterpret_cast<BatchFieldInst<FL> *>(inst->data());
    for (size_t i = 0; i < hf.size(); i++) {
        a[i].f = to_dev<FL>(hf[i]);
        a[i].quirk_mod = hf[i].quirk_mod;
        memcpy(ones->data() + i * FL, hf[i].r, 8 * FL);
    }
}

template <int FL>
int32_t launch_batch_combine_fields_fl(zip_ctx *ctx, const BatchCombineArgs &a, uint32_t n_polys, bool do_int, const void *inst_d) {
    const dim3 grid((a.row_len + kBatchCombineThreads - 1) / kBatchCombineThreads, n_polys), block(kBatchCombineThreads);
    const BatchFieldInst<FL> *inst = static_cast<const BatchFieldInst<FL> *>(inst_d);
    LaunchTimer t(ctx, "batch_combine_fields_kernel", ctx->stream);
    if (do_int) hipLaunchKernelGGL((batch_combine_fields_kernel<FL, true>), grid, block, 0, ctx->stream, a, inst);
    else hipLaunchKernelGGL((batch_combine_fields_kernel<FL, false>), grid, block, 0, ctx->stream, a, inst);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

// zip_batch_open_each: the two launches over the members [e.first, e.first + n) of a batch, into a staging slot or
// through the table of destinations (BatchEachArgs)
template <int FL>
int32_t launch_batch_combine_each_fl(zip_ctx *ctx, const BatchCombineArgs &a, uint32_t n, bool do_int, const void *inst_d,
                                     const BatchEachArgs &e) {
    const dim3 grid((a.row_len + kBatchCombineThreads - 1) / kBatchCombineThreads, n), block(kBatchCombineThreads);
    const BatchFieldInst<FL> *inst = static_cast<const BatchFieldInst<FL> *>(inst_d);
    LaunchTimer t(ctx, "batch_combine_each_kernel", ctx->stream);
    if (do_int) hipLaunchKernelGGL((batch_combine_each_kernel<FL, true>), grid, block, 0, ctx->stream, a, inst, e);
    else hipLaunchKernelGGL((batch_combine_each_kernel<FL, false>), grid, block, 0, ctx->stream, a, inst, e);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}
int32_t launch_batch_open_columns_each(zip_ctx *ctx, const BatchOpenColsArgs &g, uint32_t n, const BatchEachArgs &e) {
    // (cw <= 16384: 2 * depth + 1 <= 29 lanes per row; an image of 32 records is at most 14.6 KB)
    const size_t lds = (size_t)g.rows_per_block * (8 + 32 * (size_t)g.depth);
    const dim3 grid(g.n_cols, (g.num_rows + g.rows_per_block - 1) / g.rows_per_block, n), block(256);
    LaunchTimer t(ctx, "batch_open_columns_each_kernel", ctx->stream);
    hipLaunchKernelGGL(batch_open_columns_each_kernel<32>, grid, block, lds, ctx->stream, g, e);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}
}  // namespace

// ------------------------------------------------------------------ INT_LIMBS = 2 (kernels_two_limb.cuh)
// The single-context PCS path of a ctx created with (n_limbs, k_limbs, m_limbs) = (2, 8, 16).  The exported calls branch
// here before they reach any one-limb dispatcher.  Everything runs on ctx->stream, one launch after the other: a two-limb
// commit always materialises every row entry (Int<8>, the reference's layout) and every tree, there is no hint, no
// speculation and no chunk pipeline, so a handle is complete the moment the stream has drained (c->done stays null).
namespace {

bool two_limb(const zip_ctx *ctx) { return ctx->p.n_limbs == 2; }

// The paths that are not built for such a ctx answer ZIP_ERR_UNSUPPORTED before anything reaches the device
int32_t refuse_two_limb(zip_ctx *ctx, const char *what) {
    if (two_limb(ctx)) return fail(ctx, ZIP_ERR_UNSUPPORTED, "%s is not built for a two-limb ctx (n_limbs = 2)", what);
    return ZIP_OK;
}

// field_from_int128's qm: 2^(64 FL) - q when the modulus has its top bit set and that value is below 2^128 (only then
// can it be <= |w| for a 128-bit w), else 0
u128 tl_quirk_mod(const HostField &hf) {
    if (!(hf.modulus[hf.fl - 1] >> 63)) return 0;
    uint64_t m[8] = {0};
    sub_limbs(m, hf.modulus, hf.fl);
    for (uint32_t i = 2; i < hf.fl; i++)
        if (m[i]) return 0;
    return ((u128)m[1] << 64) | m[0];
}

// R^(i+2) mod q, i = 0 .. ceil(8 / FL) - 1: what field_from_int512 multiplies chunk i of a 512-bit magnitude by
template <int FL>
Phi8Consts<FL> tl_phi8_consts(const HostField &hf) {
    Phi8Consts<FL> pc;
    uint64_t x[8] = {0};
    memcpy(x, hf.r2, 8 * FL);
    for (int c = 0; c < Phi8Consts<FL>::N; c++) {
        if (c)
            for (int i = 0; i < 64 * FL; i++) dbl_mod(x, hf.modulus, FL);
        for (int i = 0; i < FL; i++) pc.p[c][i] = x[i];
    }
    return pc;
}

int32_t tl_commit(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind, int32_t with_merkle,
                  uint8_t *roots_out, zip_commitment **out) {
    if (!ctx || !out) return ZIP_ERR_NULL;
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    const uint32_t R = ctx->rows_local, C = ctx->p.row_len, cw = ctx->p.codeword_len;
    if (n_evals != (size_t)R * C)
        return fail(ctx, ZIP_ERR_SHAPE,
                    "Polynomial has an incorrect number of evaluations (%zu) for the expected matrix size (%zu)",
                    n_evals, (size_t)R * C);
    if (!evals) return fail(ctx, ZIP_ERR_NULL, "evals is NULL");
    zip_commitment *c = new (std::nothrow) zip_commitment();
    if (!c) return ZIP_ERR_ALLOC;
    c->ctx = ctx;
    int32_t rc = ZIP_OK;
    do {
        c->rows_bytes = (size_t)R * cw * 64;
        if ((rc = pool_alloc(ctx, c->rows_bytes, (void **)&c->rows))) break;
        if (with_merkle) {
            c->layers_bytes = (size_t)R * 2 * cw * 32;
            c->roots_bytes = (size_t)R * 32;
            if ((rc = pool_alloc(ctx, c->layers_bytes, (void **)&c->layers))) break;
            if ((rc = pool_alloc(ctx, c->roots_bytes, (void **)&c->roots))) break;
        }
        const uint64_t *evals_d = reinterpret_cast<const uint64_t *>(evals);
        if (evals_kind == ZIP_MEM_HOST) {
            c->evals_bytes = n_evals * 16;
            if ((rc = pool_alloc(ctx, c->evals_bytes, (void **)&c->evals))) break;
            if ((rc = copy_h2d_bounced(ctx, c->evals, evals, c->evals_bytes, ctx->stream))) break;
            evals_d = reinterpret_cast<const uint64_t *>(c->evals);
        }
        // Workgroups of the launch: at most four per CU (16 of the CU's 32 wave slots), and no more than keep the t1
        // scratch rows (cw * 24 bytes each) of all of them within 128 MiB, half the Infinity Cache: 1024 workgroups up to
        // cw 4096, 682 at cw 8192, 85 at cw 65536.  Whether fewer, L2-sized sets of rows would be faster was not measured.
        const uint64_t scratch_cap = ((uint64_t)128 << 20) / ((uint64_t)cw * kTlLane * 8);
        const uint32_t G = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)R, (uint64_t)ctx->num_cus * 4u, scratch_cap}));
        Scratch t1(ctx);
        if ((rc = t1.get((size_t)G * cw * kTlLane * 8))) break;
        TlEncodeArgs a{};
        a.evals = evals_d;
        a.perm1 = ctx->perm1_d;
        a.perm2 = ctx->perm2_d;
        a.t1 = t1.as<uint64_t>();
        a.rows = c->rows;
        a.layers = c->layers;
        a.num_rows = R;
        a.row_len = C;
        a.cw = cw;
        {
            LaunchTimer t(ctx, "tl_encode_rows_kernel");
            if (with_merkle) hipLaunchKernelGGL(tl_encode_rows_kernel<true>, dim3(G), dim3(256), 0, ctx->stream, a);
            else hipLaunchKernelGGL(tl_encode_rows_kernel<false>, dim3(G), dim3(256), 0, ctx->stream, a);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "tl_encode_rows_kernel: %s", hipGetErrorString(e)); break; }
        }
        if (with_merkle && (rc = merkle_upper_levels(ctx, ctx->stream, c->layers, c->roots, R, cw, 0, ctx->depth))) break;
        if (with_merkle && roots_out) {
            if ((rc = deliver(ctx, roots_out, ZIP_MEM_HOST, c->roots, c->roots_bytes))) break;
        } else if (evals_kind == ZIP_MEM_HOST) {
            hipError_t e = stream_wait(ctx->stream);
            if (e != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "two-limb commit: %s", hipGetErrorString(e)); break; }
        }
    } while (0);
    if (rc) {
        const std::string keep = ctx->last_error;
        (void)stream_wait(ctx->stream);  // nothing may still write the blocks when they return to the pool
        zip_commitment_free(c);
        ctx->last_error = keep;
        return rc;
    }
    *out = c;
    return ZIP_OK;
}

struct TlCombineOut {
    uint64_t *uprime = nullptr;     // device, [row_len][16]
    uint64_t *row_limbs = nullptr;  // device, [row_len][FL]
    uint8_t *row_be = nullptr;      // device, big-endian stream bytes
};

template <int FL>
int32_t tl_run_combine_fl(zip_ctx *ctx, TlCombineArgs a, const HostField *hf, bool do_int, bool do_field, const TlCombineOut &o) {
    const uint32_t R = a.num_rows, C = a.row_len;
    const uint32_t bx = (C + 63) / 64;
    const uint32_t by = std::max(1u, std::min((R + 3) / 4, 2048u / std::min(bx, 2048u)));
    Scratch parts(ctx);
    int32_t rc = parts.get((size_t)by * C * (kTlAcc + FL) * 8);
    if (rc) return rc;
    a.part_int = parts.as<uint64_t>();
    a.part_f = a.part_int + (size_t)by * C * kTlAcc;
    FieldDev<FL> fd{};
    if (do_field) {
        fd = to_dev<FL>(*hf);
        const u128 qm = tl_quirk_mod(*hf);
        a.qm_lo = (uint64_t)qm;
        a.qm_hi = (uint64_t)(qm >> 64);
    }
    const dim3 grid(bx, by), block(256);
    {
        LaunchTimer t(ctx, "tl_combine_kernel");
        if (do_int && do_field) hipLaunchKernelGGL((tl_combine_kernel<FL, true, true>), grid, block, 0, ctx->stream, a, fd);
        else if (do_int) hipLaunchKernelGGL((tl_combine_kernel<FL, true, false>), grid, block, 0, ctx->stream, a, fd);
        else hipLaunchKernelGGL((tl_combine_kernel<FL, false, true>), grid, block, 0, ctx->stream, a, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    LaunchTimer t(ctx, "tl_combine_finalize_kernel");
    hipLaunchKernelGGL(tl_combine_finalize_kernel<FL>, dim3((C + 255) / 256), dim3(256), 0, ctx->stream, a.part_int, a.part_f, by, C,
                       do_int ? o.uprime : nullptr, do_field ? o.row_limbs : nullptr, do_field ? o.row_be : nullptr, fd);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

// Both row combinations of a two-limb witness in one pass (either may be switched off).  Device pointers throughout.
int32_t tl_run_combine(zip_ctx *ctx, const uint64_t *evals_d, const uint64_t *coeffs_dv, const uint64_t *q0_dv, const HostField *hf,
                       bool do_int, bool do_field, const TlCombineOut &o) {
    if (!do_int && !do_field) return ZIP_OK;
    TlCombineArgs a{};
    a.evals = evals_d;
    a.coeffs = coeffs_dv;
    a.q0 = q0_dv;
    a.num_rows = ctx->rows_local;
    a.row_len = ctx->p.row_len;
    return with_fl(do_field ? hf->fl : 4u,
                   [&](auto FL) { return tl_run_combine_fl<decltype(FL)::value>(ctx, a, hf, do_int, do_field, o); });
}

int32_t tl_open_testing(zip_ctx *ctx, const int64_t *evals, zip_mem_kind evals_kind, const int64_t *coeffs, uint64_t *uprime_out,
                        zip_mem_kind out_kind) {
    Scratch ev(ctx), res(ctx), small(ctx);
    const int64_t *evals_d;
    int32_t rc;
    if ((rc = stage_evals(ctx, evals, evals_kind, (size_t)ctx->rows_local * ctx->p.row_len * 2, ev, &evals_d))) return rc;
    const size_t bytes = (size_t)ctx->p.row_len * ctx->p.m_limbs * 8;
    TlCombineOut o;
    o.uprime = uprime_out;
    if (out_kind != ZIP_MEM_DEVICE) {
        if ((rc = res.get(bytes))) return rc;
        o.uprime = res.as<uint64_t>();
    }
    SmallInputs si;
    si.src[0] = coeffs;
    si.bytes[0] = (size_t)ctx->rows_local * 16;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    if ((rc = tl_run_combine(ctx, reinterpret_cast<const uint64_t *>(evals_d), reinterpret_cast<const uint64_t *>(sb + si.off[0]),
                             nullptr, nullptr, true, false, o)))
        return rc;
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, uprime_out, ZIP_MEM_HOST, o.uprime, bytes);
    HIP_TRY(ctx, stream_wait(ctx->stream));  // coeffs were read from host memory
    return ZIP_OK;
}

// row_out != null: the evaluation row (Montgomery limbs); value_out != null: <row, q1>, the witness MLE at the point
int32_t tl_open_eval(zip_ctx *ctx, const int64_t *evals, zip_mem_kind evals_kind, const uint64_t *q0_mont, const uint64_t *q1_mont,
                     const zip_field *field, uint64_t *row_out, zip_mem_kind out_kind, uint64_t *value_out) {
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    const uint32_t R = ctx->rows_local, C = ctx->p.row_len;
    const bool single = ctx->p.num_rows == 1;
    if (!single && !q0_mont) return fail(ctx, ZIP_ERR_NULL, "q0_mont is NULL");
    if (value_out && C > 1 && !q1_mont) return fail(ctx, ZIP_ERR_NULL, "q1_mont is NULL");
    Scratch ev(ctx), res(ctx), small(ctx), dot(ctx);
    const int64_t *evals_d;
    if ((rc = stage_evals(ctx, evals, evals_kind, (size_t)R * C * 2, ev, &evals_d))) return rc;
    const size_t bytes = (size_t)C * hf.fl * 8;
    TlCombineOut o;
    o.row_limbs = row_out;
    if (!row_out || out_kind != ZIP_MEM_DEVICE) {
        if ((rc = res.get(bytes))) return rc;
        o.row_limbs = res.as<uint64_t>();
    }
    // one row: the evaluation row is map_to_field(evals) = 1_mont (x) phi(w) (open_z.rs:84-88)
    SmallInputs si;
    si.src[1] = single ? hf.r : q0_mont;
    si.bytes[1] = (size_t)R * hf.fl * 8;
    if (value_out) {
        si.src[3] = C > 1 ? (const void *)q1_mont : (const void *)hf.r;  // a one-column matrix evaluates to its entry
        si.bytes[3] = (size_t)C * hf.fl * 8;
    }
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    if ((rc = tl_run_combine(ctx, reinterpret_cast<const uint64_t *>(evals_d), nullptr, reinterpret_cast<const uint64_t *>(sb + si.off[1]),
                             &hf, false, true, o)))
        return rc;
    if (value_out) {
        if ((rc = dot.get(64))) return rc;
        {
            LaunchTimer t(ctx, "field_dot_kernel");
            const uint64_t *q1d = reinterpret_cast<const uint64_t *>(sb + si.off[3]);
            with_fl(hf.fl, [&](auto FL) {
                constexpr int N = decltype(FL)::value;
                hipLaunchKernelGGL(field_dot_kernel<N>, dim3(1), dim3(1024), 0, ctx->stream, o.row_limbs, q1d, C, dot.as<uint64_t>(),
                                   to_dev<N>(hf));
            });
            HIP_TRY(ctx, hipGetLastError());
        }
        return deliver(ctx, value_out, ZIP_MEM_HOST, dot.ptr, (size_t)hf.fl * 8);
    }
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, row_out, ZIP_MEM_HOST, o.row_limbs, bytes);
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

int32_t tl_launch_open_columns(zip_commitment *c, const uint32_t *cols_dv, uint32_t n_cols, uint8_t *out_d) {
    zip_ctx *ctx = c->ctx;
    if (!n_cols) return ZIP_OK;
    TlOpenColsArgs a{};
    a.rows = c->rows;
    a.layers = c->layers;
    a.cols = cols_dv;
    a.out = out_d;
    a.num_rows = ctx->rows_local;
    a.cw = ctx->p.codeword_len;
    a.depth = ctx->depth;
    a.n_cols = n_cols;
    const uint64_t total = (uint64_t)n_cols * a.num_rows * (a.depth + 2);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, (uint64_t)ctx->num_cus * 64);
    LaunchTimer t(ctx, "tl_open_columns_kernel");
    hipLaunchKernelGGL(tl_open_columns_kernel, dim3(blocks), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

int32_t tl_open_columns(zip_commitment *c, const uint32_t *cols, uint32_t n_cols, uint8_t *wire_out, zip_mem_kind out_kind) {
    zip_ctx *ctx = c->ctx;
    if (!c->layers) return fail(ctx, ZIP_ERR_INVALID_PARAM, "commitment has no Merkle trees (commit_no_merkle)");
    const size_t bytes = (size_t)n_cols * column_bytes(ctx);
    Scratch res(ctx), small(ctx);
    uint8_t *out_d = wire_out;
    int32_t rc;
    if (out_kind == ZIP_MEM_HOST) {
        if ((rc = res.get(bytes))) return rc;
        out_d = res.as<uint8_t>();
    }
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    SmallInputs si;
    si.src[0] = cols;
    si.bytes[0] = (size_t)n_cols * 4;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    if ((rc = tl_launch_open_columns(c, reinterpret_cast<const uint32_t *>(sb), n_cols, out_d))) return rc;
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, wire_out, ZIP_MEM_HOST, out_d, bytes);
    HIP_TRY(ctx, stream_wait(ctx->stream));  // cols were read from host memory
    return ZIP_OK;
}

// The whole stream of MultilinearZip::open into out_d (device): [u' if num_rows > 1][openings][evaluation row].
// Synchronises: the small host inputs have been consumed on return.
int32_t tl_open_device(zip_commitment *c, const uint64_t *evals_d, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols,
                       const uint64_t *q0_mont, const HostField &hf, uint8_t *out_d) {
    zip_ctx *ctx = c->ctx;
    const bool single = ctx->p.num_rows == 1;
    const size_t u_bytes = uprime_bytes(ctx), col_bytes = (size_t)n_cols * column_bytes(ctx);
    Scratch small(ctx);
    SmallInputs si;
    if (!single) {
        si.src[0] = coeffs;
        si.bytes[0] = (size_t)ctx->rows_local * 16;
    }
    si.src[1] = single ? hf.r : q0_mont;
    si.bytes[1] = (size_t)ctx->rows_local * hf.fl * 8;
    si.src[2] = cols;
    si.bytes[2] = (size_t)n_cols * 4;
    unsigned char *sb;
    int32_t rc;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    TlCombineOut o;
    o.uprime = single ? nullptr : reinterpret_cast<uint64_t *>(out_d);
    o.row_be = out_d + u_bytes + col_bytes;
    if ((rc = tl_run_combine(ctx, evals_d, reinterpret_cast<const uint64_t *>(sb + si.off[0]),
                             reinterpret_cast<const uint64_t *>(sb + si.off[1]), &hf, !single, true, o)))
        return rc;
    if ((rc = tl_launch_open_columns(c, reinterpret_cast<const uint32_t *>(sb + si.off[2]), n_cols, out_d + u_bytes))) return rc;
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

int32_t tl_open(zip_commitment *c, const int64_t *evals, zip_mem_kind evals_kind, const int64_t *coeffs, const uint32_t *cols,
                uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field, uint8_t *proof_out, zip_mem_kind out_kind) {
    zip_ctx *ctx = c->ctx;
    if (!c->layers) return fail(ctx, ZIP_ERR_INVALID_PARAM, "commitment has no Merkle trees (commit_no_merkle)");
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    if (ctx->p.num_rows > 1 && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    Scratch ev(ctx), res(ctx);
    const int64_t *evals_d = c->evals;  // witness retained by a host-side commit
    if (evals) {
        if ((rc = stage_evals(ctx, evals, evals_kind, (size_t)ctx->rows_local * ctx->p.row_len * 2, ev, &evals_d))) return rc;
    } else if (!evals_d) {
        return fail(ctx, ZIP_ERR_NULL, "evals is NULL and the commitment retains no witness");
    }
    const size_t total = zip_proof_len(ctx, n_cols, hf.fl);
    uint8_t *out_d = proof_out;
    if (out_kind == ZIP_MEM_HOST) {
        if ((rc = res.get(total))) return rc;
        out_d = res.as<uint8_t>();
    }
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    if ((rc = tl_open_device(c, reinterpret_cast<const uint64_t *>(evals_d), coeffs, cols, n_cols, q0_mont, hf, out_d))) return rc;
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, proof_out, ZIP_MEM_HOST, out_d, total);
    return ZIP_OK;
}

int32_t tl_commit_open(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                       const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field, uint8_t *roots_out,
                       uint8_t *proof_out, zip_mem_kind out_kind, zip_commitment **out) {
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    if (ctx->p.num_rows > 1 && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    const size_t total = zip_proof_len(ctx, n_cols, hf.fl);
    Scratch res(ctx);
    uint8_t *out_d = proof_out;
    if (out_kind == ZIP_MEM_HOST) {
        if ((rc = res.get(total))) return rc;
        out_d = res.as<uint8_t>();
    }
    zip_commitment *c = nullptr;
    if ((rc = tl_commit(ctx, evals, n_evals, evals_kind, 1, roots_out, &c))) return rc;
    const uint64_t *evals_d = reinterpret_cast<const uint64_t *>(c->evals ? c->evals : evals);
    rc = tl_open_device(c, evals_d, coeffs, cols, n_cols, q0_mont, hf, out_d);
    if (!rc && out_kind == ZIP_MEM_HOST) rc = deliver(ctx, proof_out, ZIP_MEM_HOST, out_d, total);
    if (rc || !out) {
        const std::string keep = ctx->last_error;
        zip_commitment_free(c);
        ctx->last_error = keep;
        return rc;
    }
    *out = c;
    return ZIP_OK;
}

template <int FL>
int32_t tl_run_verify_fl(zip_ctx *ctx, const uint8_t *proof_d, const uint64_t *coeffs_d, const uint64_t *q0_d, const uint32_t *cols_d,
                         const uint64_t *q1_d, const uint32_t *roots_d, uint32_t n_cols, const HostField &hf,
                         std::vector<uint32_t> &flags, std::vector<uint32_t> &bad, std::vector<uint32_t> &malformed, VerifyHead *cnt) {
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, cw = ctx->p.codeword_len;
    constexpr int M = 16;
    const bool single = R == 1;
    const size_t u_bytes = uprime_bytes(ctx), cols_bytes = (size_t)n_cols * column_bytes(ctx);
    Scratch enc_u(ctx), enc_f(ctx), tmp(ctx), row(ctx), misc(ctx);
    int32_t rc;
    if ((rc = enc_u.get((size_t)cw * M * 8))) return rc;
    if ((rc = enc_f.get((size_t)cw * FL * 8))) return rc;
    if ((rc = tmp.get((size_t)cw * M * 8))) return rc;
    if ((rc = row.get((size_t)C * FL * 8))) return rc;
    const size_t misc_bytes = sizeof(VerifyHead) + (size_t)3 * n_cols * 4;
    if ((rc = misc.get(misc_bytes))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(misc.ptr, 0, misc_bytes, ctx->stream));
    VerifyHead *cnt_d = misc.as<VerifyHead>();
    uint32_t *flags_d = reinterpret_cast<uint32_t *>(cnt_d + 1), *bad_d = flags_d + n_cols, *mal_d = bad_d + n_cols;
    const FieldDev<FL> fd = to_dev<FL>(hf);
    // encode_wide(u') over Int<16>, prefixes formed in 17 limbs (verify_z.rs:75-77)
    if (!single) {
        FieldDev<M> unused{};
        if ((rc = launch_encode_row<M, false>(ctx, reinterpret_cast<const uint64_t *>(proof_d), tmp.as<uint64_t>(), enc_u.as<uint64_t>(),
                                              unused, &cnt_d->overflow)))
            return rc;
    }
    {
        LaunchTimer t(ctx, "decode_field_row_kernel");
        hipLaunchKernelGGL(decode_field_row_kernel<FL>, dim3((C + 255) / 256), dim3(256), 0, ctx->stream, proof_d + u_bytes + cols_bytes,
                           C, row.as<uint64_t>(), &cnt_d->noncanonical, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    if ((rc = launch_encode_row<FL, true>(ctx, row.as<uint64_t>(), tmp.as<uint64_t>(), enc_f.as<uint64_t>(), fd, nullptr))) return rc;
    if (C > 1) {  // q_1 of a one-column matrix is empty (pcs/utils.rs:253-276): <row, q1> is 0, nothing is staged for it
        LaunchTimer t(ctx, "field_dot_kernel");
        hipLaunchKernelGGL(field_dot_kernel<FL>, dim3(1), dim3(1024), 0, ctx->stream, row.as<uint64_t>(), q1_d, C, cnt_d->dot, fd);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (n_cols) {
        TlVerifyColsArgs a{};
        a.wire = proof_d + u_bytes;
        a.cols = cols_d;
        a.coeffs = single ? nullptr : coeffs_d;
        a.q0 = single ? nullptr : q0_d;
        a.roots = roots_d;
        a.enc_int = single ? nullptr : enc_u.as<uint64_t>();
        a.enc_f = enc_f.as<uint64_t>();
        a.num_rows = R;
        a.depth = ctx->depth;
        a.n_cols = n_cols;
        a.flags = flags_d;
        a.bad_merkle = bad_d;
        a.malformed = mal_d;
        LaunchTimer t(ctx, "tl_verify_columns_kernel");
        hipLaunchKernelGGL(tl_verify_columns_kernel<FL>, dim3(n_cols), dim3(256), 0, ctx->stream, a, fd, tl_phi8_consts<FL>(hf));
        HIP_TRY(ctx, hipGetLastError());
    }
    std::vector<unsigned char> host(misc_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), misc.ptr, misc_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    memcpy(cnt, host.data(), sizeof(VerifyHead));
    const uint32_t *w = reinterpret_cast<const uint32_t *>(host.data() + sizeof(VerifyHead));
    flags.assign(w, w + n_cols);
    bad.assign(w + n_cols, w + 2 * n_cols);
    malformed.assign(w + 2 * n_cols, w + 3 * n_cols);
    return ZIP_OK;
}

// zip_verify for a two-limb ctx: the same facts, the same verdict order (verify_verdict)
int32_t tl_verify(zip_ctx *ctx, const uint8_t *roots, const uint8_t *proof, zip_mem_kind proof_kind, size_t proof_len,
                  const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const uint64_t *q1_mont,
                  const uint64_t *eval_mont, const zip_field *field, zip_verify_report *report) {
    HostField hf;
    int32_t rc;
    if ((rc = check_verify_args(ctx, coeffs, cols, n_cols, q0_mont, q1_mont, field, &hf))) return rc;
    const size_t need = zip_proof_len(ctx, n_cols, hf.fl);
    if (proof_len < need) {
        report->verdict = ZIP_VERIFY_MALFORMED;
        return ZIP_OK;
    }
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len;
    const bool single = R == 1;
    Scratch pbuf(ctx), small(ctx);
    const uint8_t *proof_d = proof;
    if (proof_kind == ZIP_MEM_HOST) {
        if ((rc = pbuf.get(need))) return rc;
        if ((rc = copy_h2d_bounced(ctx, pbuf.ptr, proof, need, ctx->stream))) return rc;
        proof_d = pbuf.as<uint8_t>();
    }
    SmallInputs si;
    si.src[0] = coeffs;  si.bytes[0] = single ? 0 : (size_t)R * 16;
    si.src[1] = q0_mont; si.bytes[1] = single ? 0 : (size_t)R * hf.fl * 8;
    si.src[2] = cols;    si.bytes[2] = (size_t)n_cols * 4;
    si.src[3] = q1_mont; si.bytes[3] = C > 1 ? (size_t)C * hf.fl * 8 : 0;
    si.src[4] = roots;   si.bytes[4] = (size_t)R * 32;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    std::vector<uint32_t> flags, bad, malformed;
    VerifyHead cnt{};
    if ((rc = with_fl(hf.fl, [&](auto FL) {
             return tl_run_verify_fl<decltype(FL)::value>(
                 ctx, proof_d, reinterpret_cast<const uint64_t *>(sb + si.off[0]), reinterpret_cast<const uint64_t *>(sb + si.off[1]),
                 reinterpret_cast<const uint32_t *>(sb + si.off[2]), reinterpret_cast<const uint64_t *>(sb + si.off[3]),
                 reinterpret_cast<const uint32_t *>(sb + si.off[4]), n_cols, hf, flags, bad, malformed, &cnt);
         })))
        return rc;
    VerifyFacts x{};
    x.overflow = cnt.overflow != 0;
    x.first = x.first_q0 = kNoOpening;
    for (uint32_t i = 0; i < n_cols; i++) {
        report->bad_merkle_paths += bad[i];
        report->malformed_paths += malformed[i];
        const uint32_t why = opening_fails(flags[i], malformed[i], bad[i]);
        if (why && x.first == kNoOpening) {
            x.first = i;
            x.first_why = why;
        }
        if ((flags[i] & 2u) && x.first_q0 == kNoOpening) x.first_q0 = i;
    }
    const uint64_t zero[4] = {0, 0, 0, 0};
    x.eval_differs = memcmp(C > 1 ? cnt.dot : zero, eval_mont, 8 * hf.fl) != 0;
    x.noncanonical = cnt.noncanonical != 0;
    verify_verdict(x, *report);
    return ZIP_OK;
}

int32_t tl_field_map_int(zip_ctx *ctx, const uint64_t *values, uint32_t n, uint32_t value_limbs, const zip_field *field, uint64_t *out) {
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    Scratch in(ctx), res(ctx);
    const size_t in_bytes = (size_t)n * value_limbs * 8;
    if ((rc = in.get(in_bytes + 16))) return rc;
    if ((rc = res.get((size_t)n * hf.fl * 8 + 16))) return rc;
    if (!n) return ZIP_OK;
    HIP_TRY(ctx, hipMemcpyAsync(in.ptr, values, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((n + 255) / 256), block(256);
    const u128 qm = tl_quirk_mod(hf);
    with_fl(hf.fl, [&](auto FL) {
        constexpr int N = decltype(FL)::value;
        if (value_limbs == 2)
            hipLaunchKernelGGL(tl_field_map_int2_kernel<N>, grid, block, 0, ctx->stream, in.as<uint64_t>(), n, res.as<uint64_t>(),
                               to_dev<N>(hf), (uint64_t)qm, (uint64_t)(qm >> 64));
        else
            hipLaunchKernelGGL(tl_field_map_int8_kernel<N>, grid, block, 0, ctx->stream, in.as<uint64_t>(), n, res.as<uint64_t>(),
                               to_dev<N>(hf), tl_phi8_consts<N>(hf));
    });
    HIP_TRY(ctx, hipGetLastError());
    return deliver(ctx, out, ZIP_MEM_HOST, res.ptr, (size_t)n * hf.fl * 8);
}

}  // namespace

extern "C" {

int32_t zip_abi_version(void) { return ZIP_HIP_ABI_VERSION; }

const char *zip_strerror(int32_t code) {
    switch (code) {
        case ZIP_OK: return "ok";
        case ZIP_ERR_INVALID_PARAM: return "invalid PCS parameter";
        case ZIP_ERR_SHAPE: return "shape mismatch (the reference panics here)";
        case ZIP_ERR_HIP: return "HIP runtime error";
        case ZIP_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
        case ZIP_ERR_UNSUPPORTED: return "unsupported geometry";
        case ZIP_ERR_ALLOC: return "device allocation failed";
        case ZIP_ERR_NULL: return "null argument";
        default: return "unknown error";
    }
}

int32_t zip_host_register(void *p, size_t bytes) {
    if (!p || !bytes) return ZIP_ERR_NULL;
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return ZIP_ERR_ALLOC;
    }
    return ZIP_OK;
}

void zip_host_unregister(void *p) {
    if (p && hipHostUnregister(p) != hipSuccess) (void)hipGetLastError();
}

void zip_release_cached_memory(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return;
    for (int d = 0; d < n && d < kMaxDevices; d++) {
        if (hipSetDevice(d) != hipSuccess) continue;
        recycle_flush(d);
        prime_dev_release(d);
    }
}

int32_t zip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int32_t zip_ctx_create(const zip_params *p, zip_ctx **out) {
    if (!p || !out) return ZIP_ERR_NULL;
    *out = nullptr;
    // ---- geometry checks (no GPU needed) ----
    // Int<1> witnesses (N, K, M = 1, 4, 8) or Int<2> witnesses (2, 8, 16); a two-limb ctx has no row shards
    const bool two = p->n_limbs == 2 && p->k_limbs == 8 && p->m_limbs == 16;
    if (!two && (p->n_limbs != 1 || p->k_limbs != 4 || p->m_limbs != 8)) return ZIP_ERR_UNSUPPORTED;
    if (two && (p->row_begin != 0 || (p->row_count != 0 && p->row_count != p->num_rows))) return ZIP_ERR_UNSUPPORTED;
    if (!is_pow2(p->row_len) || !is_pow2(p->rep) || !is_pow2(p->num_rows)) return ZIP_ERR_INVALID_PARAM;
    if ((uint64_t)p->row_len * p->rep != p->codeword_len) return ZIP_ERR_INVALID_PARAM;
    if (p->num_vars > 40 || (uint64_t)p->row_len * p->num_rows != (1ull << p->num_vars)) return ZIP_ERR_INVALID_PARAM;
    {
        // RaaCode::new width assertion, src/zip/code_raa.rs:53-72
        const uint32_t nv_even = (p->num_vars & 1) ? p->num_vars + 1 : p->num_vars;
        const uint32_t width = 64 * p->n_limbs + nv_even + 2 * ilog2(p->rep);
        if (width > 64 * p->k_limbs) return ZIP_ERR_INVALID_PARAM;
    }
    // 96-bit lanes (the width bound is 64 + 2 log2 cw at these geometries) + one workgroup per row
    if (p->codeword_len > 65536) return ZIP_ERR_UNSUPPORTED;
    if (!p->perm1 || !p->perm2) return ZIP_ERR_NULL;
    const uint32_t rows_local = p->row_count ? p->row_count : p->num_rows;
    if ((uint64_t)p->row_begin + rows_local > p->num_rows) return ZIP_ERR_INVALID_PARAM;
    {
        std::vector<uint8_t> seen(p->codeword_len);
        for (int k = 0; k < 2; k++) {
            const uint32_t *perm = k ? p->perm2 : p->perm1;
            std::fill(seen.begin(), seen.end(), 0);
            for (uint32_t j = 0; j < p->codeword_len; j++) {
                if (perm[j] >= p->codeword_len || seen[perm[j]]) return ZIP_ERR_INVALID_PARAM;
                seen[perm[j]] = 1;
            }
        }
    }
    // ---- device ----
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ZIP_ERR_NO_DEVICE;
    if (p->device < 0 || p->device >= ndev) return ZIP_ERR_NO_DEVICE;
    zip_ctx *ctx = new (std::nothrow) zip_ctx();
    if (!ctx) return ZIP_ERR_ALLOC;
    ctx->p = *p;
    ctx->p.perm1 = ctx->p.perm2 = nullptr;
    ctx->device = p->device;
    ctx->depth = ilog2(p->codeword_len);  // codeword_len.next_power_of_two().ilog2(), commit.rs:67
    ctx->rows_local = rows_local;
    if (two) ctx->speculate = 0;  // a two-limb commit stores everything: nothing to hint (zip_ctx_set_speculation keeps it off)
    int32_t rc = ZIP_OK;
    do {
        if (hipSetDevice(ctx->device) != hipSuccess) { rc = ZIP_ERR_NO_DEVICE; break; }
        // the VALU-bound producers get dispatch priority; the memory-bound consumers on `stream`
        // fill whatever wave slots / LDS the big commit workgroups leave free
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);  // numerically lower = higher priority
        if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_lo) != hipSuccess ||
            hipStreamCreateWithPriority(&ctx->s_commit, hipStreamNonBlocking, prio_hi) != hipSuccess ||
            hipStreamCreateWithPriority(&ctx->s_upper, hipStreamNonBlocking, prio_hi) != hipSuccess) {
            rc = ZIP_ERR_HIP;
            break;
        }
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0)
            ctx->num_cus = (uint32_t)cus;
        // one pinned block: [0, 4096) pipeline status words, [4096, ...) staging of small inputs
        ctx->stage_cap = (size_t)1 << 20;
        if (hipHostMalloc((void **)&ctx->pinned_base, 4096 + ctx->stage_cap, hipHostMallocDefault) != hipSuccess) {
            ctx->stage_cap = 0;
            rc = ZIP_ERR_ALLOC;
            break;
        }
        ctx->timeout_flag_h = reinterpret_cast<uint32_t *>(ctx->pinned_base);
        ctx->stage_h = ctx->pinned_base + 4096;
        if (hipHostGetDevicePointer((void **)&ctx->timeout_flag_d, ctx->timeout_flag_h, 0) != hipSuccess) {
            rc = ZIP_ERR_ALLOC;
            break;
        }
        *ctx->timeout_flag_h = 0;
        ctx->clock_h = reinterpret_cast<unsigned long long *>(ctx->pinned_base + 256);
        memset(ctx->clock_h, 0, 32);
        if (hipHostGetDevicePointer((void **)&ctx->clock_d, ctx->clock_h, 0) != hipSuccess) {
            rc = ZIP_ERR_ALLOC;
            break;
        }
        // pipeline chunks: the persistent commit kernel publishes its rows in this many groups
        // (0 = chosen per commit from the number of rounds; ZIP_HIP_CHUNKS overrides)
        ctx->n_chunks = (uint32_t)env_long("ZIP_HIP_CHUNKS", 0, 1, 64);
        // the other knobs of the chunk schedule and of the gather (zip_ctx): read here, never by a call
        ctx->knob_rpb = (uint32_t)env_long("ZIP_HIP_GATHER_RPB", 0, 2, 4096);
        ctx->knob_stream = (int)env_long("ZIP_HIP_GATHER_STREAM", -1, 0, 1);
        if (const char *e = getenv("ZIP_HIP_CHUNK_ROUNDS")) ctx->knob_chunk_rounds = e;
        ctx->no_compact = getenv("ZIP_HIP_NO_COMPACT_ROWS") != nullptr;
        const size_t pb = (size_t)p->codeword_len * 4;
        if (hipMalloc((void **)&ctx->perm1_d, pb) != hipSuccess || hipMalloc((void **)&ctx->perm2_d, pb) != hipSuccess) {
            rc = ZIP_ERR_ALLOC;
            break;
        }
        if (hipMemcpy(ctx->perm1_d, p->perm1, pb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(ctx->perm2_d, p->perm2, pb, hipMemcpyHostToDevice) != hipSuccess) {
            rc = ZIP_ERR_HIP;
            break;
        }
    } while (0);
    if (rc) {
        zip_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return ZIP_OK;
}

void zip_ctx_destroy(zip_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->s_commit) (void)stream_wait(ctx->s_commit);
    if (ctx->s_upper) (void)stream_wait(ctx->s_upper);
    if (ctx->stream) (void)stream_wait(ctx->stream);
    ctx->hint_plan.reset();  // (its device block goes back to the pool that is torn down next)
    *ctx->alive = false;
    if (ctx->recycle) {
        for (auto &kv : ctx->free_blocks) recycle_give(ctx->device, kv.first, kv.second);
        for (auto &kv : ctx->live_blocks) recycle_give(ctx->device, kv.second, kv.first);
    } else {
        for (auto &kv : ctx->free_blocks) (void)hipFree(kv.second);
        for (auto &kv : ctx->live_blocks) (void)hipFree(kv.first);
    }
    for (auto &pe : ctx->pending) {
        (void)hipEventDestroy(pe.start);
        (void)hipEventDestroy(pe.stop);
    }
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    for (auto e : ctx->dep_event_pool) (void)hipEventDestroy(e);
    if (ctx->s_commit) (void)hipStreamDestroy(ctx->s_commit);
    if (ctx->s_upper) (void)hipStreamDestroy(ctx->s_upper);
    if (ctx->stage_big) (void)hipHostFree(ctx->stage_big);
    for (auto *h : ctx->hint_free) (void)hipHostFree(h);
    for (auto *h : ctx->job_stage)
        if (h) (void)hipHostFree(h);
    if (ctx->ring_d) (void)hipFree(ctx->ring_d);
    if (ctx->slab_d) (void)hipFree(ctx->slab_d);
    if (ctx->pinned_base) (void)hipHostFree(ctx->pinned_base);
    if (ctx->recycle && ctx->bounce[0] && ctx->bounce[1] && ctx->device >= 0 && ctx->device < kMaxDevices) {
        RecycleBin &bin = g_recycle[ctx->device];
        std::lock_guard<std::mutex> g(bin.mu);
        if (!bin.bounce_cap) {
            for (int i = 0; i < 2; i++) {
                bin.bounce[i] = ctx->bounce[i];
                ctx->bounce[i] = nullptr;
            }
            bin.bounce_cap = ctx->bounce_cap;
        }
    }
    for (auto *b : ctx->bounce)
        if (b) (void)hipHostFree(b);
    if (ctx->perm1_d) (void)hipFree(ctx->perm1_d);
    if (ctx->perm2_d) (void)hipFree(ctx->perm2_d);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *zip_ctx_last_error(const zip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int32_t zip_ctx_synchronize(zip_ctx *ctx) {
    if (!ctx) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (ctx->s_commit) HIP_TRY(ctx, stream_wait(ctx->s_commit));
    if (ctx->s_upper) HIP_TRY(ctx, stream_wait(ctx->s_upper));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return check_timeout(ctx);
}

void *zip_ctx_stream(zip_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

#ifdef ZIPK_DEBUG_STAMPS
// Debug build only (tools/wg_spread.py): one pinned, host-mapped block every commit kernel stamps into.
constexpr size_t kDebugStampWords = (size_t)kStampRec * 2048;
static unsigned long long *debug_stamps_buffer() {
    static unsigned long long *buf = nullptr;
    if (!buf && hipHostMalloc((void **)&buf, kDebugStampWords * 8, hipHostMallocDefault) == hipSuccess) memset(buf, 0, kDebugStampWords * 8);
    return buf;
}
extern "C" unsigned long long *zip_debug_stamps(uint32_t *words_per_wg) {
    if (words_per_wg) *words_per_wg = kStampRec;
    return debug_stamps_buffer();
}
#endif

static int32_t commit_impl(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind,
                           int32_t with_merkle, const uint32_t *hint_cols, uint32_t n_hint, uint8_t *roots_out,
                           zip_commitment **out) {
    if (!ctx || !out) return ZIP_ERR_NULL;
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    const uint32_t R = ctx->rows_local, C = ctx->p.row_len, cw = ctx->p.codeword_len;
    if (n_evals != (size_t)R * C)
        return fail(ctx, ZIP_ERR_SHAPE,
                    "Polynomial has an incorrect number of evaluations (%zu) for the expected matrix size (%zu)",
                    n_evals, (size_t)R * C);
    zip_commitment *c = new (std::nothrow) zip_commitment();
    if (!c) return ZIP_ERR_ALLOC;
    c->ctx = ctx;
    int32_t rc = ZIP_OK;
    do {
        // A commit that will be opened keeps 16-byte row entries in HBM (half the row stores; the gather expands them
        // on the way into the proof); encode_rows / commit_no_merkle is read back and stays Int<4>.
        c->compact_rows = with_merkle && !ctx->no_compact;
        c->rows_bytes = (size_t)R * cw * (c->compact_rows ? 16 : 32);
        {
            // packed openings take the place of the 16-byte row entries; where a row's packed block is larger than they
            // are (cw <= 4096 with 1000 openings) the buffer is sized for it
            size_t alloc = c->rows_bytes;
            if (with_merkle && hint_cols && commit_supports_hint(cw)) {
                const auto plan = get_hint_plan(ctx, hint_cols, n_hint, c->compact_rows && n_hint && packed_enabled());
                // (packed blocks and the tree levels beside them are interleaved in groups of four rows: CommitArgs.pk)
                if (plan->packed) alloc = std::max(alloc, (size_t)((R + 3u) & ~3u) * plan->L.stride);
            }
            if ((rc = pool_alloc(ctx, alloc, (void **)&c->rows))) break;
        }
        if (with_merkle) {
            c->layers_bytes = (size_t)R * 2 * cw * 32;
            c->roots_bytes = (size_t)R * 32;
            // (whole groups of four rows: a packed commit stores its trees row-interleaved)
            if ((rc = pool_alloc(ctx, (size_t)((R + 3u) & ~3u) * 2 * cw * 32, (void **)&c->layers))) break;
            if ((rc = pool_alloc(ctx, c->roots_bytes, (void **)&c->roots))) break;
        }
        const int64_t *evals_d = evals;
        if (!evals) { rc = fail(ctx, ZIP_ERR_NULL, "evals is NULL"); break; }
        if (evals_kind == ZIP_MEM_HOST) {
            c->evals_bytes = n_evals * 8;
            if ((rc = pool_alloc(ctx, c->evals_bytes, (void **)&c->evals))) break;
            if ((rc = copy_h2d_bounced(ctx, c->evals, evals, c->evals_bytes, ctx->s_commit))) break;
            evals_d = c->evals;
        }
        // ---- ONE persistent commit launch on s_commit; its chunks are consumed on s_upper ----
        const CommitGeom geom = commit_geom(cw, C);
        uint32_t G = ctx->num_cus * commit_wgs_per_cu(geom);
        if (G > R) G = R;
        // (A commit whose rows all fit ONE round of resident workgroups -- 2^20: 1024 rows, four 256-thread workgroups
        // per CU -- has nothing to pipeline.  Half the workgroups and two rounds was tried: the kernel takes 240 instead
        // of 131 us, a round of 2 workgroups per CU lasts as long as one of 4 -- latency-bound at that size.)
        const uint32_t rounds = (R + G - 1) / G;
        // rows_per_chunk also batches the in-kernel upper tree levels, so keep it even without
        // chunk signalling (commit_no_merkle has neither)
        // default: chunks of four rounds (measured best at 2^22 / 2^23 / 2^24: 1 / 2 / 4 chunks) -- fewer
        // rounds per chunk starve the batched upper levels, more leave the gather too little to overlap
        // (few rounds -- 2^20 .. 2^22, or an eighth of 2^24 in a zip_mctx shard -- : two chunks, so that there is an overlap)
        uint32_t nch = !with_merkle ? 1 : ctx->n_chunks ? ctx->n_chunks : rounds >= 8 ? std::min(8u, rounds / 4) : rounds >= 2 ? 2u : 1u;
        if (nch > rounds) nch = rounds;
        const uint32_t rpc = (rounds + nch - 1) / nch;
        nch = (rounds + rpc - 1) / rpc;
        // chunk schedule in rounds: equal chunks, or (ZIP_HIP_CHUNK_ROUNDS="8,4,2,1,1", <= 64 rounds) an explicit one
        // whose last entry is stretched / cut to the number of rounds
        std::vector<uint32_t> sched;
        if (with_merkle && rounds <= 64) {
            const char *env = ctx->knob_chunk_rounds.empty() ? nullptr : ctx->knob_chunk_rounds.c_str();
            if (env && !ctx->n_chunks) {
                uint32_t used = 0;
                for (const char *q = env; *q && used < rounds;) {
                    char *endp = nullptr;
                    const long v = strtol(q, &endp, 10);
                    if (endp == q) break;
                    if (v >= 1) {
                        const uint32_t take = std::min<uint32_t>((uint32_t)v, rounds - used);
                        sched.push_back(take);
                        used += take;
                    }
                    q = (*endp == ',') ? endp + 1 : endp;
                }
                if (!sched.empty() && used < rounds) sched.back() += rounds - used;
            }
            // default from 12 rounds up (2^24: 16 rounds): chunks of three rounds, the remainder in the last one
            // (3,3,3,3,4).  The chain of gathers is what ends a step (each takes about as long as the commit kernel
            // needs for its chunk), so it should start early: against four chunks of four the first gather starts a
            // round earlier; a fifth chunk end costs the commit kernel ~17 us.  1.849 against 1.859-1.872 ms per step.
            // From 24 rounds (2^26: 32 rounds of the 16-entry kernel, whose chunk-end stage is full with two rows):
            // chunks of two rounds, at most 16 -- there the gathers have slack (each waits ~0.3 ms for its chunk) and
            // what ends a step is the last chunk's gather alone: 5.733 / 5.693 against 5.805 / 5.782 ms per step.
            // Round 4, 12..23 rounds (the branch-free gather, kernels_open.cuh, takes ~50 us per round beside the commit
            // kernel's ~86): the same number of chunks but DESCENDING -- a last chunk of two thirds of the base, what that
            // leaves spread over the first ones: 4,4,3,3,2 at 2^24.  What ends a step is the last chunk's gather alone
            // (29 us per round of 256 rows); the chunk before it must be gathered by the time the last one is published
            // (50 n <= 86 m: 4,4,4,3,1 and 6,4,3,2,1 lose what they gain).  Alternated on one box, four times each:
            // 1.480 / 1.485 / 1.495 / 1.543 against 1.510 / 1.528 / 1.528 / 1.579 ms for 3,3,3,3,4 (profiles/EXPERIMENTS.md).
            if (sched.empty() && !ctx->n_chunks && rounds >= 12) {
                const uint32_t n = rounds >= 24 ? std::min(kRingChunks, rounds / 2) : std::min(8u, rounds / 3), base = rounds / n;
                if (rounds >= 24 || base < 3) {
                    for (uint32_t k = 0; k + 1 < n; k++) sched.push_back(base);
                    sched.push_back(rounds - base * (n - 1));
                } else {
                    const uint32_t last = base * 2 / 3;
                    uint32_t extra = rounds - (base * (n - 1) + last);
                    for (uint32_t k = 0; k + 1 < n; k++) {
                        const uint32_t more = (extra + (n - 2 - k)) / (n - 1 - k);  // (the larger shares first)
                        sched.push_back(base + more);
                        extra -= more;
                    }
                    sched.push_back(last);
                }
            }
        }
        uint64_t chunk_ends = 0;
        if (sched.empty()) {
            for (uint32_t k = 0; k < nch; k++) sched.push_back(std::min(rpc, rounds - k * rpc));
        } else {
            nch = (uint32_t)sched.size();
            uint32_t r = 0;
            for (uint32_t k = 0; k < nch; k++) {
                r += sched[k];
                chunk_ends |= 1ull << (r - 1);
            }
        }
        c->bounds.resize(nch + 1);
        {
            uint64_t r = 0;
            for (uint32_t k = 0; k <= nch; k++) {
                const uint64_t b = r * G;
                c->bounds[k] = b < R ? (uint32_t)b : R;
                if (k < nch) r += sched[k];
            }
        }
        // ONE round of workgroups that share their CUs (2^20: 1024 rows, four 256-thread workgroups per CU) has no later
        // round for a gather to run beside: the workgroups are split into classes at different wave priorities instead
        // (CommitArgs.classes) -- class c, a contiguous c-th part of the rows, finishes and is published while the
        // later classes still hash, and its openings are gathered beside them.  Measured at 2^20 (round 4, one box,
        // twice each): two classes 0.273 / 0.278, four 0.276 / 0.277, none 0.283 / 0.283 ms per step -- the priorities
        // stagger the classes less than hoped (class 0 of four is published at 116 of the kernel's 157 us,
        // profiles/EXPERIMENTS.md), so the gain is the one gather that overlaps.  Default two; ZIP_HIP_CLASSES=1: off.
        uint32_t classes = 1;
        {
            const long knob_classes = env_long("ZIP_HIP_CLASSES", 0, 1, 64);  // (per call: the tests flip it)
            const uint32_t per_cu = commit_wgs_per_cu(geom);
            if (with_merkle && hint_cols && commit_supports_hint(cw) && rounds == 1 && R == G && per_cu >= 2 && G % 8 == 0 &&
                !ctx->n_chunks && knob_classes != 1) {
                classes = knob_classes > 1 ? (uint32_t)knob_classes : std::min(2u, per_cu);
                while (classes > 1 && ((G / 8) % classes || classes > per_cu)) classes--;
            }
            if (classes > 1) {
                nch = classes;
                chunk_ends = 0;
                c->bounds.resize(nch + 1);
                for (uint32_t k = 0; k <= nch; k++) c->bounds[k] = k * (G / classes);
            }
        }
        CommitArgs a{};
        a.classes = classes;
        a.evals = evals_d;
        a.perm1 = ctx->perm1_d;
        a.perm2 = ctx->perm2_d;
        a.rows = c->rows;
        a.compact_rows = c->compact_rows ? 1u : 0u;
        a.layers = c->layers;
        a.row_len = C;
        a.cw = cw;
        a.num_rows = R;
        a.rounds_per_chunk = rpc;
        a.chunk_ends = chunk_ends;
        a.roots = c->roots;
        a.clock = ctx->profiling ? ctx->clock_d : nullptr;
#ifdef ZIPK_DEBUG_STAMPS
        a.stamps = debug_stamps_buffer();
#endif
        hipError_t e = hipSuccess;
        if (with_merkle && hint_cols && commit_supports_hint(cw)) {
            // the hint bitmaps (CommitArgs.need): V | N0 | N1 | N2, see kernels_commit.cuh
            const uint32_t wv = (cw + 31) / 32, w1 = (cw / 2 + 31) / 32, w2 = (cw / 4 + 31) / 32;
            const size_t words = 2 * (size_t)wv + w1 + w2;
            if (words * 4 > kHintBytes) { rc = fail(ctx, ZIP_ERR_UNSUPPORTED, "hint bitmaps exceed their staging block"); break; }
            const bool want_packed = c->compact_rows && n_hint && packed_enabled();
            c->plan = get_hint_plan(ctx, hint_cols, n_hint, want_packed);
            const bool resident = c->plan->dev != nullptr;  // the tables already sit on the device (HintPlan::dev)
            if (!resident) {  // per-commit staging block + upload: there is no device copy of the plan
                if (!ctx->hint_free.empty()) {
                    c->hint_h = ctx->hint_free.back();
                    ctx->hint_free.pop_back();
                } else if (hipHostMalloc((void **)&c->hint_h, kHintBytes, hipHostMallocDefault) != hipSuccess) {
                    c->hint_h = nullptr;
                    rc = fail(ctx, ZIP_ERR_ALLOC, "hipHostMalloc(%zu) failed", kHintBytes);
                    break;
                }
            }
            uint32_t *bm = resident ? nullptr : reinterpret_cast<uint32_t *>(c->hint_h);
            if (bm) memcpy(bm, c->plan->bm.data(), words * 4);
            const uint32_t *nv = c->plan->bm.data();
            c->hint_cols.assign(nv, nv + wv);
            size_t upload = words * 4;
            if (c->plan->packed) {
                if (!resident) {
                    memcpy(c->hint_h + kHintTables, c->plan->rank_tab.data(), c->plan->rank_tab.size() * 4);
                    memcpy(c->hint_h + kPackedRanksAt, c->plan->own_ranks.data(), c->plan->own_ranks.size() * 2);
                }
                upload = kPackedRanksAt + c->plan->own_ranks.size() * 2;
                c->packed = true;
                c->pk_stride = c->plan->L.stride;
                for (int k = 0; k < 3; k++) c->pk_off[k] = c->plan->L.off[k];
            }
            const unsigned char *tables_d;
            if (resident) {
                tables_d = c->plan->dev;
            } else {
                if ((rc = pool_alloc(ctx, kHintBytes, (void **)&c->need_d))) break;
                e = hipMemcpyAsync(c->need_d, bm, upload, hipMemcpyHostToDevice, ctx->s_commit);
                if (e != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "hint upload failed: %s", hipGetErrorString(e)); break; }
                tables_d = reinterpret_cast<const unsigned char *>(c->need_d);
            }
            a.need = reinterpret_cast<const uint32_t *>(tables_d);
            c->hinted = true;
            if (c->packed) {
                a.pk = reinterpret_cast<uint8_t *>(c->rows);
                a.pk_stride = c->pk_stride;
                a.pk_off0 = c->pk_off[0];
                a.pk_off1 = c->pk_off[1];
                a.pk_off2 = c->pk_off[2];
                // (HintPlan::rank_tab: per lane for the 8-entry kernel, per wave and output phase for the 16-entry one)
                a.pk_tab = reinterpret_cast<const uint32_t *>(tables_d + kHintTables);
                c->rank_d = reinterpret_cast<const uint16_t *>(tables_d + kPackedRanksAt);
            }
        }
        // (a single chunk is published through its counter too: the gather then starts ~5 us after the commit kernel's
        // last workgroup has published instead of a cross-stream event's ~20 us after the kernel has ended -- 2^20)
        if (with_merkle && (nch > 1 || (hint_cols && R >= ctx->num_cus))) {
            if (nch <= kRingChunks && !ctx->ring_d) {  // first pipelined commit of this ctx
                if (hipMalloc((void **)&ctx->ring_d, (size_t)kRingSlots * kRingStride * 4) != hipSuccess ||
                    hipMemset(ctx->ring_d, 0, (size_t)kRingSlots * kRingStride * 4) != hipSuccess) {
                    if (ctx->ring_d) (void)hipFree(ctx->ring_d);
                    ctx->ring_d = nullptr;
                    (void)hipGetLastError();
                }
            }
            if (nch <= kRingChunks && ctx->ring_d) {
                if (ctx->ring_next == kRingSlots) {
                    // every slot has been used: nobody may still poll one (the streams are idle between calls; a kept
                    // handle notices the new epoch), then one memset for the next kRingSlots commits
                    if (e == hipSuccess) e = stream_wait(ctx->stream);
                    if (e == hipSuccess) e = stream_wait(ctx->s_commit);
                    if (e == hipSuccess) e = hipMemsetAsync(ctx->ring_d, 0, (size_t)kRingSlots * kRingStride * 4, ctx->s_commit);
                    if (e == hipSuccess) e = stream_wait(ctx->s_commit);
                    ctx->ring_next = 0;
                    ctx->ring_epoch++;
                }
                c->chunk_done = ctx->ring_d + (size_t)ctx->ring_next++ * kRingStride;
                c->ring_slot = true;
                c->ring_epoch = ctx->ring_epoch;
            } else {
                if ((rc = pool_alloc(ctx, (size_t)nch * 4, (void **)&c->chunk_done))) break;
                e = hipMemsetAsync(c->chunk_done, 0, (size_t)nch * 4, ctx->s_commit);
                c->zeroed = take_dep_event(ctx);
                if (e == hipSuccess) e = hipEventRecord(c->zeroed, ctx->s_commit);
            }
            a.chunk_done = c->chunk_done;
            c->expected.resize(nch);
            for (uint32_t k = 0; k < nch; k++) c->expected[k] = (R - c->bounds[k]) < G ? (R - c->bounds[k]) : G;
            if (classes > 1)  // (a class is G / classes workgroups, each with one row)
                for (uint32_t k = 0; k < nch; k++) c->expected[k] = G / classes;
        }
        if (e != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "commit setup failed: %s", hipGetErrorString(e)); break; }
        if (geom.e > 16) {  // raa_commit_slab_kernel: a slab per workgroup, kept by the ctx
            const size_t need = (size_t)G * cw * 16;
            if (ctx->slab_bytes < need) {
                // (an earlier commit kernel may still read the old slab)
                if (ctx->slab_d && (e = stream_wait(ctx->s_commit)) != hipSuccess) {
                    rc = fail(ctx, ZIP_ERR_HIP, "commit setup failed: %s", hipGetErrorString(e));
                    break;
                }
                if (ctx->slab_d) (void)hipFree(ctx->slab_d);
                ctx->slab_d = nullptr;
                ctx->slab_bytes = 0;
                if (hipMalloc((void **)&ctx->slab_d, need) != hipSuccess) {
                    ctx->slab_d = nullptr;
                    (void)hipGetLastError();
                    rc = fail(ctx, ZIP_ERR_ALLOC, "hipMalloc(%zu) of the commit slabs failed", need);
                    break;
                }
                ctx->slab_bytes = need;
            }
            a.slab = ctx->slab_d;
        }
        rc = with_merkle ? dispatch_commit<true>(ctx, a, G, ctx->s_commit) : dispatch_commit<false>(ctx, a, G, ctx->s_commit);
        if (rc) break;
        c->args = a;
        c->grid = G;
        c->evals_ref = evals_d;
        c->done = take_dep_event(ctx);
        e = hipEventRecord(c->done, ctx->s_commit);
        if (e != hipSuccess) rc = fail(ctx, ZIP_ERR_HIP, "commit pipeline failed: %s", hipGetErrorString(e));
        if (rc) break;
        if (with_merkle && roots_out) {
            if ((rc = wait_ready(c, ctx->stream))) break;
            if ((rc = deliver(ctx, roots_out, ZIP_MEM_HOST, c->roots, c->roots_bytes))) break;
        }
        if (evals_kind == ZIP_MEM_HOST) {
            hipError_t e = stream_wait(ctx->s_commit);  // the caller's buffer is free to go
            if (e != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "commit failed: %s", hipGetErrorString(e)); break; }
        }
    } while (0);
    if (rc) {
        zip_commitment_free(c);
        return rc;
    }
    *out = c;
    return ZIP_OK;
}

static int32_t launch_witness_digest(zip_ctx *ctx, const int64_t *evals_d, size_t n, unsigned long long *out_d, hipStream_t st);

// The two calls of an UNCHANGED ZincProver (src/zinc/prover.rs:315-320: commit, then open on a fresh PcsTranscript):
// the commit cannot be told the columns, but in that flow they never change -- they are a function of the field and
// the codeword length -- so a ctx that has seen an opening hints its next plain commits with THAT column list.  The
// open that follows finds exactly what it reads (byte-identical proof, the hinted commit's speed); anything else asked
// of the handle completes it first, transparently (rematerialize).  By default only for HOST witnesses (what the Rust
// binding passes: the library re-runs from its OWN copy, the contract of zip_commit is untouched); for DEVICE witnesses
// only after zip_ctx_set_speculation(ctx, 1) -- the handle then reads the caller's array again when it is completed
// (round-3 advisor finding: that lifetime rule must not arrive unasked).  zip_ctx_set_speculation(ctx, 0) or
// ZIP_HIP_SPECULATE=0 switches it off altogether.
int32_t zip_commit(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind,
                   int32_t with_merkle, uint8_t *roots_out, zip_commitment **out) {
    if (!ctx || !out) return ZIP_ERR_NULL;
    if (two_limb(ctx)) return tl_commit(ctx, evals, n_evals, evals_kind, with_merkle, roots_out, out);
    std::shared_ptr<HintPlan> plan;
    {
        std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
        if (with_merkle && (ctx->speculate == 2 || (ctx->speculate == 1 && evals_kind == ZIP_MEM_HOST)) && ctx->seen_columns &&
            ctx->hint_plan && ctx->hint_plan->cw == ctx->p.codeword_len &&
            !ctx->hint_plan->cols.empty() && commit_supports_hint(ctx->p.codeword_len))
            plan = ctx->hint_plan;
    }
    if (!plan) return commit_impl(ctx, evals, n_evals, evals_kind, with_merkle, nullptr, 0, roots_out, out);
    int32_t rc = commit_impl(ctx, evals, n_evals, evals_kind, 1, plan->cols.data(), (uint32_t)plan->cols.size(), roots_out, out);
    if (rc) return rc;
    zip_commitment *c = *out;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    c->speculative = true;
    if (c->hinted && !c->evals && c->evals_ref) {  // a DEVICE witness of the caller's: its digest, beside the commit kernel
        if (pool_alloc(ctx, 16, (void **)&c->digest_d) == ZIP_OK) {
            const size_t n = (size_t)ctx->rows_local * ctx->p.row_len;
            if (launch_witness_digest(ctx, c->evals_ref, n, c->digest_d, ctx->s_upper) == ZIP_OK) {
                c->digest_done = take_dep_event(ctx);
                (void)hipEventRecord(c->digest_done, ctx->s_upper);
            }
        }
    }
    return ZIP_OK;
}

int32_t zip_ctx_set_speculation(zip_ctx *ctx, int32_t on) {
    if (!ctx) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (two_limb(ctx)) return ZIP_OK;  // stays off: such a commit has no hinted form
    ctx->speculate = on ? 2 : 0;
    return ZIP_OK;
}

int32_t zip_ctx_set_proximity_tests(zip_ctx *ctx, uint32_t n_tests) {
    if (!ctx) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (n_tests < 1 || n_tests > 8)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "num_proximity_testing %u is outside the supported range 1 .. 8", n_tests);
    if (n_tests > 1 && two_limb(ctx)) return refuse_two_limb(ctx, "more than one proximity test");
    if (n_tests > 1 && ctx->rows_local != ctx->p.num_rows)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "a row-sharded ctx serves one proximity test (got %u)", n_tests);
    ctx->n_tests = n_tests;
    return ZIP_OK;
}
uint32_t zip_ctx_proximity_tests(const zip_ctx *ctx) { return ctx ? ctx->n_tests : 0; }

int32_t zip_commit_hinted(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind,
                          const uint32_t *cols, uint32_t n_cols, uint8_t *roots_out, zip_commitment **out) {
    if (!ctx || !out) return ZIP_ERR_NULL;
    if (n_cols && !cols) return ZIP_ERR_NULL;
    {
        std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
        if (int32_t rc = check_cols(ctx, cols, n_cols)) return rc;
    }
    // (a two-limb commit ignores the hint: it stores every entry and every node)
    if (two_limb(ctx)) return tl_commit(ctx, evals, n_evals, evals_kind, 1, roots_out, out);
    static const uint32_t none = 0;
    return commit_impl(ctx, evals, n_evals, evals_kind, 1, cols ? cols : &none, n_cols, roots_out, out);
}

// A hinted commitment is asked for something its kernel did not store: run the commit again, in full, into the
// same buffers (same witness, same tables: the same bits where they already exist), and wait for it.
static int32_t launch_witness_digest(zip_ctx *ctx, const int64_t *evals_d, size_t n, unsigned long long *out_d, hipStream_t st) {
    HIP_TRY(ctx, hipMemsetAsync(out_d, 0, 16, st));
    const uint32_t blocks = (uint32_t)std::min<size_t>((n / 2 + 255) / 256, (size_t)ctx->num_cus);
    hipLaunchKernelGGL(witness_digest_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, reinterpret_cast<const uint64_t *>(evals_d),
                       (uint64_t)n, out_d);
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

// `evals_now`: the witness as the CURRENT call was handed it (zip_open gets the polynomial again), or null
static int32_t rematerialize(zip_commitment *c, const int64_t *evals_now = nullptr) {
    if (!c->hinted) return ZIP_OK;
    zip_ctx *ctx = c->ctx;
    CommitArgs a = c->args;
    a.need = nullptr;
    a.pk = nullptr;
    a.clock = nullptr;
    a.chunk_done = nullptr;  // the chunks of the first run stay published
    a.evals = evals_now ? evals_now : c->evals ? c->evals : c->evals_ref;
    if (a.evals == c->evals_ref && !c->evals && c->speculative && c->digest_d) {
        // the caller's device array, read a second time without the caller having been told it would be: has it changed?
        const size_t n = (size_t)ctx->rows_local * ctx->p.row_len;
        Scratch again(ctx);
        int32_t rc = again.get(16);
        if (rc) return rc;
        if (c->digest_done) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, c->digest_done, 0));
        if ((rc = launch_witness_digest(ctx, c->evals_ref, n, again.as<unsigned long long>(), ctx->stream))) return rc;
        unsigned long long then_[2] = {0, 0}, now_[2] = {1, 1};
        HIP_TRY(ctx, hipMemcpyAsync(then_, c->digest_d, 16, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(now_, again.ptr, 16, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, stream_wait(ctx->stream));
        if (then_[0] != now_[0] || then_[1] != now_[1])
            return fail(ctx, ZIP_ERR_INVALID_PARAM,
                        "the device witness of this commitment has changed since zip_commit: the handle only holds what an "
                        "opening of the ctx's usual columns reads (speculative hint) and cannot be completed any more; keep the "
                        "witness until the handle is freed, or switch the speculation off (zip_ctx_set_speculation)");
    }
    if (c->done) HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_commit, c->done, 0));
    HIP_TRY(ctx, stream_wait(ctx->stream));  // nobody still gathers from the buffers
    int32_t rc = dispatch_commit<true>(ctx, a, c->grid, ctx->s_commit);
    if (rc) return rc;
    if (c->done) HIP_TRY(ctx, hipEventRecord(c->done, ctx->s_commit));
    HIP_TRY(ctx, stream_wait(ctx->s_commit));
    c->hinted = false;
    c->packed = false;
    return ZIP_OK;
}

// every column of cols[] lies inside the hint (host check); otherwise the handle is completed first
static int32_t ensure_columns(zip_commitment *c, const uint32_t *cols, uint32_t n_cols, const int64_t *evals_now = nullptr) {
    if (!c->hinted) return ZIP_OK;
    // ... a packed handle serves the openings it was hinted with, in their order (rank_d); anything else completes it
    if (c->packed)
        return (c->plan && c->plan->cols.size() == n_cols && (n_cols == 0 || !memcmp(c->plan->cols.data(), cols, (size_t)n_cols * 4)))
                   ? ZIP_OK : rematerialize(c, evals_now);
    for (uint32_t i = 0; i < n_cols; i++) {
        const uint32_t col = cols[i];
        if ((col >> 5) >= c->hint_cols.size() || !((c->hint_cols[col >> 5] >> (col & 31)) & 1u)) return rematerialize(c, evals_now);
    }
    return ZIP_OK;
}

// An opening names the columns this ctx's prover squeezes: the next plain zip_commit hints itself with them.
static void note_columns(zip_ctx *ctx, const uint32_t *cols, uint32_t n_cols) {
    if (!ctx->speculate || !n_cols || !commit_supports_hint(ctx->p.codeword_len)) return;
    (void)get_hint_plan(ctx, cols, n_cols, !ctx->no_compact && packed_enabled());
    ctx->seen_columns = true;
}

void zip_commitment_free(zip_commitment *c) {
    if (!c) return;
    std::lock_guard<std::recursive_mutex> api_lock(c->ctx->api_mu);
    // nothing may still be reading or writing the buffers when they return to the pool
    if (c->done) {
        (void)event_wait(c->done);
        c->ctx->dep_event_pool.push_back(c->done);
    }
    if (c->zeroed) c->ctx->dep_event_pool.push_back(c->zeroed);
    for (hipEvent_t e : c->aux) c->ctx->dep_event_pool.push_back(e);
    if (c->ctx->stream && !c->consumers_done) (void)stream_wait(c->ctx->stream);
    if (!c->ring_slot) pool_release(c->ctx, c->chunk_done);
    if (c->digest_done) {
        (void)event_wait(c->digest_done);
        c->ctx->dep_event_pool.push_back(c->digest_done);
    }
    pool_release(c->ctx, c->digest_d);
    pool_release(c->ctx, c->need_d);
    if (c->hint_h) c->ctx->hint_free.push_back(c->hint_h);
    if (!c->borrows_rows) pool_release(c->ctx, c->rows);
    if (!c->borrows_rest) {
        pool_release(c->ctx, c->layers);
        pool_release(c->ctx, c->roots);
        pool_release(c->ctx, c->evals);
    }
    delete c;  // (a batch member: drops its reference to the batch's storage)
}

static int32_t materialize_rows(zip_commitment *c);

int32_t zip_commitment_device_ptrs(zip_commitment *c, uint64_t **rows, uint8_t **layers, uint8_t **roots) {
    if (!c) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(c->ctx->api_mu);
    // work enqueued on the ctx stream (zip_ctx_stream) after this call sees complete data
    int32_t rc_ = (rows || layers) ? rematerialize(c) : ZIP_OK;
    if (rc_) return rc_;
    if ((rc_ = wait_ready(c, c->ctx->stream))) return rc_;
    if (rows) {
        if ((rc_ = materialize_rows(c))) return rc_;
        *rows = c->rows;
    }
    if (layers) *layers = reinterpret_cast<uint8_t *>(c->layers);
    if (roots) *roots = reinterpret_cast<uint8_t *>(c->roots);
    return ZIP_OK;
}

// One-way: the compact rows of a commitment become the Int<4> array the ABI promises to whoever looks at them
// (zip_commit_download, zip_commitment_device_ptrs); afterwards the handle behaves like an uploaded one.
static int32_t materialize_rows(zip_commitment *c) {
    if (!c->compact_rows) return ZIP_OK;
    zip_ctx *ctx = c->ctx;
    int32_t rc = wait_ready(c, ctx->stream);
    if (rc) return rc;
    const uint64_t n = c->rows_bytes / 16;
    void *full = nullptr;
    if ((rc = pool_alloc(ctx, (size_t)n * 32, &full))) return rc;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 65535);
    hipLaunchKernelGGL(expand_rows_kernel, dim3(blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const uint4 *>(c->rows),
                       static_cast<uint4 *>(full), n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = stream_wait(ctx->stream);
    if (e != hipSuccess) {
        (void)stream_wait(ctx->stream);  // nothing may still write `full` when it returns to the pool
        pool_release(ctx, full);
        return fail(ctx, ZIP_ERR_HIP, "expanding the row entries failed: %s", hipGetErrorString(e));
    }
    if (!c->borrows_rows) pool_release(ctx, c->rows);
    c->borrows_rows = false;
    c->rows = static_cast<uint64_t *>(full);
    c->rows_bytes = (size_t)n * 32;
    c->compact_rows = false;
    return ZIP_OK;
}

int32_t zip_commit_download(zip_commitment *c, uint64_t *rows_out, uint8_t *layers_out, uint8_t *roots_out) {
    if (!c) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    const uint32_t R = ctx->rows_local, cw = ctx->p.codeword_len;
    {
        int32_t rc_ = (rows_out || layers_out) ? rematerialize(c) : ZIP_OK;
        if (rc_) return rc_;
        if ((rc_ = wait_ready(c, ctx->stream))) return rc_;
    }
    if (rows_out) {
        int32_t rc_ = materialize_rows(c);
        if (rc_) return rc_;
        rc_ = copy_d2h_bounced(ctx, rows_out, c->rows, c->rows_bytes, ctx->stream);
        if (rc_) return rc_;
    }
    if (layers_out) {
        if (!c->layers) return fail(ctx, ZIP_ERR_INVALID_PARAM, "commitment has no Merkle trees (commit_no_merkle)");
        const size_t w = ((size_t)2 * cw - 2) * 32;
        if (w)
            HIP_TRY(ctx, hipMemcpy2DAsync(layers_out, w, c->layers, (size_t)2 * cw * 32, w, R, hipMemcpyDeviceToHost,
                                          ctx->stream));
    }
    if (roots_out) {
        if (!c->roots) return fail(ctx, ZIP_ERR_INVALID_PARAM, "commitment has no Merkle roots (commit_no_merkle)");
        HIP_TRY(ctx, hipMemcpyAsync(roots_out, c->roots, c->roots_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

int32_t zip_commitment_upload(zip_ctx *ctx, const uint64_t *rows, const uint8_t *layers, const uint8_t *roots,
                              zip_commitment **out) {
    if (!ctx || !out || !rows) return ZIP_ERR_NULL;
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    const uint32_t R = ctx->rows_local, cw = ctx->p.codeword_len;
    zip_commitment *c = new (std::nothrow) zip_commitment();
    if (!c) return ZIP_ERR_ALLOC;
    c->ctx = ctx;
    int32_t rc = ZIP_OK;
    do {
        c->rows_bytes = (size_t)R * cw * 8 * ctx->p.k_limbs;  // Int<4> entries, Int<8> on a two-limb ctx
        if ((rc = pool_alloc(ctx, c->rows_bytes, (void **)&c->rows))) break;
        hipError_t e = hipMemcpyAsync(c->rows, rows, c->rows_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && layers) {
            c->layers_bytes = (size_t)R * 2 * cw * 32;
            c->roots_bytes = (size_t)R * 32;
            // (whole groups of four rows: a packed commit stores its trees row-interleaved)
            if ((rc = pool_alloc(ctx, (size_t)((R + 3u) & ~3u) * 2 * cw * 32, (void **)&c->layers))) break;
            if ((rc = pool_alloc(ctx, c->roots_bytes, (void **)&c->roots))) break;
            const size_t w = ((size_t)2 * cw - 2) * 32;
            if (w) e = hipMemcpy2DAsync(c->layers, (size_t)2 * cw * 32, layers, w, w, R, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess && roots) {
                e = hipMemcpyAsync(c->roots, roots, c->roots_bytes, hipMemcpyHostToDevice, ctx->stream);
                // keep the in-tree root slot consistent with the separate roots array
                if (e == hipSuccess)
                    e = hipMemcpy2DAsync(reinterpret_cast<uint8_t *>(c->layers) + ((size_t)2 * cw - 2) * 32,
                                         (size_t)2 * cw * 32, roots, 32, 32, R, hipMemcpyHostToDevice, ctx->stream);
            }
        }
        if (e == hipSuccess) e = stream_wait(ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, ZIP_ERR_HIP, "upload failed: %s", hipGetErrorString(e));
    } while (0);
    if (rc) {
        zip_commitment_free(c);
        return rc;
    }
    *out = c;
    return ZIP_OK;
}

int32_t zip_open_testing(zip_ctx *ctx, const int64_t *evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                         uint64_t *uprime_out, zip_mem_kind out_kind) {
    if (!ctx || !coeffs || !uprime_out) return ZIP_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (two_limb(ctx)) return tl_open_testing(ctx, evals, evals_kind, coeffs, uprime_out, out_kind);
    Scratch ev(ctx), res(ctx);
    const int64_t *evals_d;
    int32_t rc;
    if ((rc = stage_evals(ctx, evals, evals_kind, (size_t)ctx->rows_local * ctx->p.row_len, ev, &evals_d))) return rc;
    const uint32_t T = proximity_tests(ctx);
    const size_t bytes = (size_t)T * ctx->p.row_len * ctx->p.m_limbs * 8;
    CombineOut o{};
    if (out_kind == ZIP_MEM_DEVICE) {
        o.uprime = uprime_out;
    } else {
        if ((rc = res.get(bytes))) return rc;
        o.uprime = res.as<uint64_t>();
    }
    Scratch small(ctx);
    SmallInputs si;
    si.src[0] = coeffs;
    si.bytes[0] = (size_t)T * ctx->rows_local * 8;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    const int64_t *coeffs_dv = reinterpret_cast<const int64_t *>(sb + si.off[0]);
    if ((rc = run_combine(ctx, evals_d, coeffs_dv, nullptr, nullptr, true, false, o))) return rc;
    if ((rc = run_combine_extra(ctx, evals_d, coeffs_dv + ctx->rows_local, T - 1,
                                o.uprime + (size_t)ctx->p.row_len * ctx->p.m_limbs)))
        return rc;
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, uprime_out, ZIP_MEM_HOST, o.uprime, bytes);
    HIP_TRY(ctx, stream_wait(ctx->stream));  // coeffs were read from host memory
    return ZIP_OK;
}

int32_t zip_open_columns(zip_commitment *c, const uint32_t *cols, uint32_t n_cols, uint8_t *wire_out,
                         zip_mem_kind out_kind) {
    if (!c || !cols || !wire_out) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (two_limb(ctx)) return tl_open_columns(c, cols, n_cols, wire_out, out_kind);
    if (!c->layers) return fail(ctx, ZIP_ERR_INVALID_PARAM, "commitment has no Merkle trees (commit_no_merkle)");
    const size_t bytes = (size_t)n_cols * column_bytes(ctx);
    Scratch res(ctx);
    uint8_t *out_d = wire_out;
    int32_t rc;
    if (out_kind == ZIP_MEM_HOST) {
        if ((rc = res.get(bytes))) return rc;
        out_d = res.as<uint8_t>();
    }
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    if ((rc = ensure_columns(c, cols, n_cols))) return rc;
    Scratch small(ctx);
    SmallInputs si;
    si.src[0] = cols;
    si.bytes[0] = (size_t)n_cols * 4;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    if ((rc = run_open_columns_pipelined(c, reinterpret_cast<const uint32_t *>(sb), n_cols, out_d))) return rc;
    if ((rc = recover_gather_timeout(c, reinterpret_cast<const uint32_t *>(sb), n_cols, out_d))) return rc;  // (synchronises)
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, wire_out, ZIP_MEM_HOST, out_d, bytes);
    return ZIP_OK;
}

int32_t zip_open_eval(zip_ctx *ctx, const int64_t *evals, zip_mem_kind evals_kind, const uint64_t *q0_mont,
                      const zip_field *field, uint64_t *row_out, zip_mem_kind out_kind) {
    if (!ctx || !row_out) return ZIP_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (two_limb(ctx)) return tl_open_eval(ctx, evals, evals_kind, q0_mont, nullptr, field, row_out, out_kind, nullptr);
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    const bool single = ctx->p.num_rows == 1;
    if (!single && !q0_mont) return fail(ctx, ZIP_ERR_NULL, "q0_mont is NULL");
    Scratch ev(ctx), res(ctx);
    const int64_t *evals_d;
    if ((rc = stage_evals(ctx, evals, evals_kind, (size_t)ctx->rows_local * ctx->p.row_len, ev, &evals_d))) return rc;
    const size_t bytes = (size_t)ctx->p.row_len * hf.fl * 8;
    CombineOut o{};
    if (out_kind == ZIP_MEM_DEVICE) {
        o.row_limbs = row_out;
    } else {
        if ((rc = res.get(bytes))) return rc;
        o.row_limbs = res.as<uint64_t>();
    }
    // one row: the evaluation row is map_to_field(evals) = 1_mont * w (open_z.rs:84-88)
    Scratch small(ctx);
    SmallInputs si;
    si.src[1] = single ? hf.r : q0_mont;
    si.bytes[1] = (size_t)ctx->rows_local * hf.fl * 8;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    if ((rc = run_combine(ctx, evals_d, nullptr, reinterpret_cast<const uint64_t *>(sb + si.off[1]), &hf, false, true,
                          o)))
        return rc;
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, row_out, ZIP_MEM_HOST, o.row_limbs, bytes);
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

size_t zip_proof_len(const zip_ctx *ctx, uint32_t n_cols, uint32_t field_limbs) {
    if (!ctx) return 0;
    size_t len = 0;
    len += uprime_bytes(ctx);
    len += (size_t)n_cols * column_bytes(ctx);
    len += (size_t)ctx->p.row_len * field_limbs * 8;
    return len;
}

// The body of MultilinearZip::open with everything on the device: row combinations, column openings (pipelined behind
// the commit kernel), evaluation row -> out_d.  open_enqueue puts all of it on the streams (OpenState holds what must
// outlive the launches), open_finish waits for it; open_device is the two together.
struct OpenState {
    Scratch small;
    const uint32_t *cols_dv = nullptr;
    uint32_t n_cols = 0;
    uint8_t *openings_d = nullptr;
    explicit OpenState(zip_ctx *c) : small(c) {}
};
constexpr size_t kJobStageBytes = (size_t)1 << 20;
// What open_enqueue stages for one job (its SmallInputs, each rounded to 256 bytes as stage_small lays them out: the
// proximity coefficients, q0, the columns, their gather order and the packed gather table -- counted whether or not
// the commit turns out packed), at least kJobStageBytes.  2^30 with a 4-limb field: 32768 rows x 40 bytes = 1.3 MB.
static size_t job_stage_bytes(const zip_ctx *ctx, uint32_t n_cols, uint32_t fl) {
    auto r = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const bool single = ctx->p.num_rows == 1;
    size_t t = (single ? 0 : r((size_t)proximity_tests(ctx) * ctx->rows_local * 8)) + r((size_t)ctx->rows_local * fl * 8) + r((size_t)n_cols * 4);
    if (n_cols > 1) t += r((size_t)n_cols * 4);
    if (n_cols <= 65536) t += r((size_t)n_cols * 16);
    return std::max(t, kJobStageBytes);
}

static int32_t open_enqueue(zip_commitment *c, const int64_t *evals_d, const int64_t *coeffs, const uint32_t *cols,
                            uint32_t n_cols, const uint64_t *q0_mont, const HostField &hf, uint8_t *out_d, OpenState &st,
                            unsigned char *own_stage = nullptr, size_t own_cap = 0) {
    zip_ctx *ctx = c->ctx;
    int32_t rc;
    const bool single = ctx->p.num_rows == 1;
    const uint32_t T = proximity_tests(ctx);
    const size_t u_bytes = uprime_bytes(ctx);  // u'_0 .. u'_{T-1}
    const size_t col_bytes = (size_t)n_cols * column_bytes(ctx);
    CombineOut o{};
    o.uprime = single ? nullptr : reinterpret_cast<uint64_t *>(out_d);
    o.row_be = out_d + u_bytes + col_bytes;
    Scratch &small = st.small;
    SmallInputs si;
    if (!single) {
        si.src[0] = coeffs;  // [T][num_rows], test-major
        si.bytes[0] = (size_t)T * ctx->rows_local * 8;
    }
    si.src[1] = single ? hf.r : q0_mont;
    si.bytes[1] = (size_t)ctx->rows_local * hf.fl * 8;
    si.src[2] = cols;
    si.bytes[2] = (size_t)n_cols * 4;
    std::vector<uint32_t> order;
    if (n_cols > 1) {
        order.resize(n_cols);
        gather_order(cols, n_cols, order.data());
        si.src[3] = order.data();
        si.bytes[3] = (size_t)n_cols * 4;
    }
    // packed handles: what gather workgroup x needs (opening, column, the four packed ranks) in one 16-byte entry
    std::vector<uint32_t> wg_tab;
    if (c->packed && c->plan && c->plan->cols.size() == n_cols && c->plan->own_ranks.size() == (size_t)n_cols * 4 && n_cols <= 65536) {
        wg_tab.resize((size_t)n_cols * 4);
        for (uint32_t b = 0; b < n_cols; b++) {
            const uint32_t i = order.empty() ? b : order[b];
            const uint16_t *r = c->plan->own_ranks.data() + (size_t)i * 4;
            wg_tab[4 * b] = i | (cols[i] << 16);
            wg_tab[4 * b + 1] = (uint32_t)r[0] | ((uint32_t)r[1] << 16);
            wg_tab[4 * b + 2] = (uint32_t)r[2] | ((uint32_t)r[3] << 16);
            wg_tab[4 * b + 3] = 0;
        }
        si.src[4] = wg_tab.data();
        si.bytes[4] = wg_tab.size() * 4;
    }
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb, own_stage, own_cap))) return rc;
    c->gather_order = order.empty() ? nullptr : reinterpret_cast<const uint32_t *>(sb + si.off[3]);  // (lives in `small`)
    c->gather_tab = wg_tab.empty() ? nullptr : reinterpret_cast<const uint4 *>(sb + si.off[4]);
    st.cols_dv = reinterpret_cast<const uint32_t *>(sb + si.off[2]);
    st.n_cols = n_cols;
    st.openings_d = out_d + u_bytes;
    // The two row combinations do not depend on the commitment: both kernels go on the main stream ahead of the
    // gathers -- the stream would otherwise idle until the commit kernel publishes its first chunk, and with s_setprio
    // they are not starved by the hashing waves: 0.07 + 0.02 ms there (round 3's kernels: 64 / 77 VGPRs and 9 KB of
    // LDS, both fit beside the commit workgroups).  1.676 / 1.718 / 1.725 against 1.710 / 1.732 / 1.735 ms per step
    // for the fold of the partial sums last, alternated on one box.  (The other placements -- the fold last, both on
    // a stream of their own, held back until the commit kernel ends, or after the gathers -- were removed:
    // EXPERIMENTS.md.)
    const int64_t *coeffs_dv = reinterpret_cast<const int64_t *>(sb + si.off[0]);
    const uint64_t *q0_dv = reinterpret_cast<const uint64_t *>(sb + si.off[1]);
    if ((rc = run_combine(ctx, evals_d, coeffs_dv, q0_dv, &hf, !single, true, o))) return rc;
    // tests 1 .. T-1: one more pass over the witness behind them, same stream, same wave priority
    if (T > 1 && (rc = run_combine_extra(ctx, evals_d, coeffs_dv + ctx->rows_local, T - 1,
                                         o.uprime + (size_t)ctx->p.row_len * ctx->p.m_limbs)))
        return rc;
    return run_open_columns_pipelined(c, st.cols_dv, n_cols, st.openings_d);
}
// synchronises: the small host inputs (coeffs, cols, q0) have been consumed, every launch has run
static int32_t open_finish(zip_commitment *c, OpenState &st, bool force_regather = false) {
    const int32_t rc = recover_gather_timeout(c, st.cols_dv, st.n_cols, st.openings_d, force_regather);
    c->gather_order = nullptr;  // the tables live in st.small
    c->gather_tab = nullptr;
    return rc;
}
static int32_t open_device(zip_commitment *c, const int64_t *evals_d, const int64_t *coeffs, const uint32_t *cols,
                           uint32_t n_cols, const uint64_t *q0_mont, const HostField &hf, uint8_t *out_d) {
    OpenState st(c->ctx);
    int32_t rc = open_enqueue(c, evals_d, coeffs, cols, n_cols, q0_mont, hf, out_d, st);
    if (rc) {
        c->gather_order = nullptr;
        c->gather_tab = nullptr;
        return rc;
    }
    return open_finish(c, st);
}

int32_t zip_open(zip_commitment *c, const int64_t *evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                 const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field,
                 uint8_t *proof_out, zip_mem_kind out_kind) {
    if (!c || !proof_out || (n_cols && !cols)) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (two_limb(ctx)) return tl_open(c, evals, evals_kind, coeffs, cols, n_cols, q0_mont, field, proof_out, out_kind);
    if (ctx->rows_local != ctx->p.num_rows)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_open needs an unsharded ctx; use the per-phase calls on a row shard");
    if (!c->layers) return fail(ctx, ZIP_ERR_INVALID_PARAM, "commitment has no Merkle trees (commit_no_merkle)");
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    const bool single = ctx->p.num_rows == 1;
    if (!single && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    Scratch ev(ctx), res(ctx);
    const int64_t *evals_d = c->evals;  // witness retained by a host-side commit
    if (evals) {
        if ((rc = stage_evals(ctx, evals, evals_kind, (size_t)ctx->rows_local * ctx->p.row_len, ev, &evals_d))) return rc;
    } else if (!evals_d) {
        return fail(ctx, ZIP_ERR_NULL, "evals is NULL and the commitment retains no witness");
    }
    const size_t total = zip_proof_len(ctx, n_cols, hf.fl);
    uint8_t *out_d = proof_out;
    if (out_kind == ZIP_MEM_HOST) {
        if ((rc = res.get(total))) return rc;
        out_d = res.as<uint8_t>();
    }
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    if ((rc = ensure_columns(c, cols, n_cols, evals_d))) return rc;
    note_columns(ctx, cols, n_cols);
    if ((rc = open_device(c, evals_d, coeffs, cols, n_cols, q0_mont, hf, out_d))) return rc;
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, proof_out, ZIP_MEM_HOST, out_d, total);
    return ZIP_OK;
}

// The open of ONE ROW SHARD in one call (what zip_mctx does per shard, for the one-process-per-GPU arrangement of
// zinc_amd/dist.py): one pass over the shard's witness rows for both partial row combinations, and the shard's rows of
// every opened column, pipelined behind its commit kernel.  Everything DEVICE memory, asynchronous on the ctx's stream
// except the small host inputs (consumed on return: the call synchronises the stream once).
int32_t zip_open_shard(zip_commitment *c, const int64_t *evals_d, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols,
                       const uint64_t *q0_mont, const zip_field *field, uint64_t *uprime_part_d, uint64_t *row_part_d,
                       uint8_t *wire_d) {
    if (!c || !evals_d || !wire_d || !row_part_d || (n_cols && !cols)) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (int32_t r = refuse_two_limb(ctx, "zip_open_shard")) return r;
    if (!c->layers) return fail(ctx, ZIP_ERR_INVALID_PARAM, "commitment has no Merkle trees (commit_no_merkle)");
    HostField hf;
    int32_t rc;
    if ((rc = refuse_extra_tests(ctx, "zip_open_shard"))) return rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    const bool single = ctx->p.num_rows == 1;
    if (!single && (!coeffs || !q0_mont || !uprime_part_d)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont / uprime_part is NULL");
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    if ((rc = ensure_columns(c, cols, n_cols, evals_d))) return rc;
    Scratch small(ctx);
    CombineScratch cscr(ctx);
    SmallInputs si;
    if (!single) {
        si.src[0] = coeffs;
        si.bytes[0] = (size_t)ctx->rows_local * 8;
    }
    si.src[1] = single ? hf.r : q0_mont;
    si.bytes[1] = (size_t)ctx->rows_local * hf.fl * 8;
    si.src[2] = cols;
    si.bytes[2] = (size_t)n_cols * 4;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    const uint32_t *cols_dv = reinterpret_cast<const uint32_t *>(sb + si.off[2]);
    CombineOut o{};
    o.uprime = single ? nullptr : uprime_part_d;
    o.row_limbs = row_part_d;
    const int64_t *coeffs_dv = reinterpret_cast<const int64_t *>(sb + si.off[0]);
    const uint64_t *q0_dv = reinterpret_cast<const uint64_t *>(sb + si.off[1]);
    if ((rc = run_combine(ctx, evals_d, coeffs_dv, q0_dv, &hf, !single, true, o, &cscr, 1))) return rc;
    if ((rc = run_open_columns_pipelined(c, cols_dv, n_cols, wire_d))) return rc;
    if ((rc = run_combine(ctx, evals_d, coeffs_dv, q0_dv, &hf, !single, true, o, &cscr, 2))) return rc;
    return recover_gather_timeout(c, cols_dv, n_cols, wire_d);  // (synchronises the stream)
}

int32_t zip_commit_open(zip_ctx *ctx, const int64_t *evals, size_t n_evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                        const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field,
                        uint8_t *roots_out, uint8_t *proof_out, zip_mem_kind out_kind, zip_commitment **out) {
    if (!ctx || !proof_out || (n_cols && !cols)) return ZIP_ERR_NULL;
    if (out) *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (two_limb(ctx))
        return tl_commit_open(ctx, evals, n_evals, evals_kind, coeffs, cols, n_cols, q0_mont, field, roots_out, proof_out, out_kind, out);
    if (ctx->rows_local != ctx->p.num_rows)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_commit_open needs an unsharded ctx");
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    const bool single = ctx->p.num_rows == 1;
    if (!single && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    const size_t total = zip_proof_len(ctx, n_cols, hf.fl);
    Scratch res(ctx);
    uint8_t *out_d = proof_out;
    if (out_kind == ZIP_MEM_HOST) {
        if ((rc = res.get(total))) return rc;
        out_d = res.as<uint8_t>();
    }
    static const uint32_t none = 0;
    zip_commitment *c = nullptr;
    if ((rc = commit_impl(ctx, evals, n_evals, evals_kind, 1, cols ? cols : &none, n_cols, nullptr, &c)))
        return rc;
    const int64_t *evals_d = c->evals ? c->evals : c->evals_ref;
    rc = open_device(c, evals_d, coeffs, cols, n_cols, q0_mont, hf, out_d);
    if (!rc && roots_out) {
        rc = wait_ready(c, ctx->stream);
        if (!rc) rc = deliver(ctx, roots_out, ZIP_MEM_HOST, c->roots, c->roots_bytes);
    }
    if (!rc && out_kind == ZIP_MEM_HOST) rc = deliver(ctx, proof_out, ZIP_MEM_HOST, out_d, total);
    if (rc || !out) {
        // (the error text of `rc` must survive the calls made while freeing)
        const std::string keep = ctx->last_error;
        zip_commitment_free(c);
        ctx->last_error = keep;
        return rc;
    }
    *out = c;
    return ZIP_OK;
}

// ---- zip_commit_open as a job: begin enqueues, wait collects (include/zip_hip.h) ---------------------------------
struct zip_job {
    zip_ctx *ctx = nullptr;
    zip_commitment *c = nullptr;
    OpenState *st = nullptr;
    hipEvent_t finished = nullptr;  // behind the last launch of the open on the main stream
    int slot = -1;
    uint64_t epoch = 0;  // zip_ctx::recover_epoch when the job was enqueued
};
int32_t zip_commit_open_begin(zip_ctx *ctx, const int64_t *evals_d, size_t n_evals, const int64_t *coeffs, const uint32_t *cols,
                              uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field, uint8_t *proof_out_d,
                              zip_job **out) {
    if (!ctx || !out || !proof_out_d || !evals_d || (n_cols && !cols)) return ZIP_ERR_NULL;
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (int32_t r = refuse_two_limb(ctx, "zip_commit_open_begin")) return r;
    if (ctx->rows_local != ctx->p.num_rows) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_commit_open_begin needs an unsharded ctx");
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    const bool single = ctx->p.num_rows == 1;
    if (!single && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    int slot = !ctx->job_busy[0] ? 0 : !ctx->job_busy[1] ? 1 : -1;
    if (slot < 0) return fail(ctx, ZIP_ERR_INVALID_PARAM, "two jobs are already in flight on this ctx: zip_job_wait one first");
    // the slot's staging block holds this job's small inputs: sized BEFORE the commit is enqueued (a free slot's block
    // is idle -- its last job has been waited for)
    const size_t stage_need = job_stage_bytes(ctx, n_cols, hf.fl);
    if (ctx->job_stage[slot] && ctx->job_stage_cap[slot] < stage_need) {
        (void)hipHostFree(ctx->job_stage[slot]);
        ctx->job_stage[slot] = nullptr;
        ctx->job_stage_cap[slot] = 0;
    }
    if (!ctx->job_stage[slot]) {
        if (hipHostMalloc((void **)&ctx->job_stage[slot], stage_need, hipHostMallocDefault) != hipSuccess) {
            ctx->job_stage[slot] = nullptr;
            return fail(ctx, ZIP_ERR_ALLOC, "hipHostMalloc(%zu) failed", stage_need);
        }
        ctx->job_stage_cap[slot] = stage_need;
    }
    zip_job *j = new (std::nothrow) zip_job();
    if (!j) return ZIP_ERR_ALLOC;
    j->ctx = ctx;
    static const uint32_t none = 0;
    if ((rc = commit_impl(ctx, evals_d, n_evals, ZIP_MEM_DEVICE, 1, cols ? cols : &none, n_cols, nullptr, &j->c))) {
        delete j;
        return rc;
    }
    j->st = new (std::nothrow) OpenState(ctx);
    if (!j->st) rc = ZIP_ERR_ALLOC;
    if (!rc)
        rc = open_enqueue(j->c, evals_d, coeffs, cols, n_cols, q0_mont, hf, proof_out_d, *j->st, ctx->job_stage[slot],
                          ctx->job_stage_cap[slot]);
    if (!rc) {
        j->finished = take_dep_event(ctx);
        if (hipEventRecord(j->finished, ctx->stream) != hipSuccess) rc = fail(ctx, ZIP_ERR_HIP, "hipEventRecord failed");
    }
    if (rc) {  // (the destructors drain what was enqueued)
        const std::string keep = ctx->last_error;
        j->c->gather_order = nullptr;
        j->c->gather_tab = nullptr;
        delete j->st;
        zip_commitment_free(j->c);
        if (j->finished) ctx->dep_event_pool.push_back(j->finished);
        delete j;
        ctx->last_error = keep;
        return rc;
    }
    ctx->job_busy[slot] = true;
    j->slot = slot;
    j->epoch = ctx->recover_epoch;
    *out = j;
    return ZIP_OK;
}

int32_t zip_job_wait(zip_job *j, uint8_t *roots_out) {
    if (!j) return ZIP_ERR_NULL;
    zip_ctx *ctx = j->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    int32_t rc = ZIP_OK;
    hipError_t e = event_wait(j->finished);  // NOT the stream: the next job may already be queued behind this one
    if (e != hipSuccess) rc = fail(ctx, ZIP_ERR_HIP, "job failed: %s", hipGetErrorString(e));
    const bool forced = j->epoch < ctx->recover_epoch;  // a recovery ran (and cleared the flag) after this job was enqueued
    if (!rc && ((ctx->timeout_flag_h && *ctx->timeout_flag_h) || forced)) {
        // a pipeline wait gave up (counter collection serialises the streams): everything in flight is redone.  The
        // first job to notice drains the streams and clears the flag; a job that was already queued then cannot tell
        // any more whether ITS waits gave up too, so it re-gathers unconditionally.  Jobs enqueued after the recovery
        // are not affected (the flag covers their own waits): no sticky state.
        rc = open_finish(j->c, *j->st, forced);  // (synchronises the streams)
    }
    if (!rc && roots_out) {
        // on s_upper, ordered after this job's commit only: the main stream may already hold the NEXT job's whole open
        if (!(rc = wait_ready(j->c, ctx->s_upper))) rc = copy_d2h_bounced(ctx, roots_out, j->c->roots, j->c->roots_bytes, ctx->s_upper);
    }
    // everything of this job on the main stream has run: nothing to drain, nothing to wait for
    const std::string keep = ctx->last_error;
    j->c->gather_order = nullptr;
    j->c->gather_tab = nullptr;
    if (!rc) j->c->consumers_done = true;
    delete j->st;
    zip_commitment_free(j->c);
    ctx->dep_event_pool.push_back(j->finished);
    ctx->job_busy[j->slot] = false;
    ctx->last_error = keep;
    delete j;
    return rc;
}

// =====================================================================================================
// Batches: many small polynomials on one ctx (the reference's batch_commit / batch_open, commit.rs:134-142,
// open_z.rs:43-58).  Every row has its own Merkle tree, so to the commit kernels B polynomials of R rows are B * R
// rows: ONE launch of the kernel a single commit of this geometry takes, everything stored, nothing hinted, no chunk
// published.  The open is two launches whatever B is (kernels_batch.cuh): the polynomial is a grid dimension.
// The verifier's side, batch_verify_z (verify_z.rs:40-58), is zip_batch_verify beside zip_verify below: five launches
// whatever B is (kernels_batch_verify.cuh), the verdicts folded on the device, B reports copied back.
// =====================================================================================================
// Process-wide (zip_batch_codes_counts): zip_batch_commit_codes calls that reached the device, the members they committed,
// and the calls of zip_batch_open_eval_fields / zip_batch_open_fields that reached the device
static std::atomic<uint64_t> g_batch_codes_commits{0}, g_batch_codes_members{0}, g_batch_field_opens{0};

// zip_batch_commit (codes == false: the ctx's permutations for every member) and zip_batch_commit_codes (perms1 / perms2:
// HOST, one slice of codeword_len entries per member)
static int32_t batch_commit_impl(zip_ctx *ctx, const int64_t *evals, size_t n_evals, uint32_t n_polys, zip_mem_kind evals_kind,
                                 bool codes, const uint32_t *perms1, const uint32_t *perms2, uint8_t *roots_out, zip_batch **out) {
    if (!ctx || !evals || !out) return ZIP_ERR_NULL;
    *out = nullptr;
    if (codes && (!perms1 || !perms2)) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (int32_t r = refuse_two_limb(ctx, codes ? "zip_batch_commit_codes" : "zip_batch_commit")) return r;
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, cw = ctx->p.codeword_len;
    if (n_polys == 0 || n_polys > 65535)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "a batch holds 1 .. 65535 polynomials (got %u)", n_polys);
    if (ctx->rows_local != R) return fail(ctx, ZIP_ERR_INVALID_PARAM, "batches need an unsharded ctx");
    if (codes && cw > kMaxCodesCodeword)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "a code per member is built for codewords up to %u: the geometry of codeword %u is "
                    "not built", kMaxCodesCodeword, cw);
    if (cw > 16384)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "batches serve codewords up to 16384 (got %u): larger polynomials are not launch-bound, "
                    "use zip_commit_open_begin", cw);
    if ((uint64_t)n_polys * R > 0xFFFFFFFFull)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "%u polynomials of %u rows exceed 2^32 rows", n_polys, R);
    if (n_evals != (size_t)n_polys * R * C)
        return fail(ctx, ZIP_ERR_SHAPE, "A batch of %u polynomials has an incorrect number of evaluations (%zu) for the expected "
                    "matrix size (%zu each)", n_polys, n_evals, (size_t)R * C);
    if (codes) {  // zip_ctx_create's test of a permutation, per member
        std::vector<uint8_t> seen(cw);
        for (uint32_t i = 0; i < n_polys; i++)
            for (int k = 0; k < 2; k++) {
                const uint32_t *perm = (k ? perms2 : perms1) + (size_t)i * cw;
                std::fill(seen.begin(), seen.end(), 0);
                for (uint32_t j = 0; j < cw; j++) {
                    if (perm[j] >= cw || seen[perm[j]])
                        return fail(ctx, ZIP_ERR_INVALID_PARAM, "member %u: perm%d is not a permutation of [0, %u)", i, k + 1, cw);
                    seen[perm[j]] = 1;
                }
            }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (codes) {
        g_batch_codes_commits++;
        g_batch_codes_members += n_polys;
    }
    const uint32_t total = n_polys * R;
    zip_batch *b = new (std::nothrow) zip_batch();
    if (!b) return ZIP_ERR_ALLOC;
    b->ctx = ctx;
    b->n_polys = n_polys;
    b->store = std::make_shared<BatchStore>();
    {
        std::shared_ptr<bool> alive = ctx->alive;  // (storage that outlives its ctx must not touch the ctx's pool)
        b->store->release = [ctx, alive](BatchStore &s) {
            if (!*alive) return;
            std::lock_guard<std::recursive_mutex> lock(ctx->api_mu);
            // nothing may still be reading or writing the blocks when they return to the pool
            (void)stream_wait(ctx->s_commit);
            (void)stream_wait(ctx->stream);
            pool_release(ctx, s.rows);
            pool_release(ctx, s.layers);
            pool_release(ctx, s.roots);
            pool_release(ctx, s.evals);
            pool_release(ctx, s.perms);
        };
    }
    BatchStore &S = *b->store;
    int32_t rc = ZIP_OK;
    do {
        if ((rc = pool_alloc(ctx, (size_t)total * cw * 16, &S.rows))) break;
        if ((rc = pool_alloc(ctx, (size_t)total * 2 * cw * 32, &S.layers))) break;
        if ((rc = pool_alloc(ctx, (size_t)total * 32, &S.roots))) break;
        b->evals_d = evals;
        if (evals_kind == ZIP_MEM_HOST) {
            if ((rc = pool_alloc(ctx, n_evals * 8, &S.evals))) break;
            if ((rc = copy_h2d_bounced(ctx, S.evals, evals, n_evals * 8, ctx->s_commit))) break;
            b->evals_d = static_cast<const int64_t *>(S.evals);
        }
        const size_t perm_words = (size_t)n_polys * cw;
        if (codes) {  // every member's permutations, once: all perm1 slices, then all perm2 slices
            if ((rc = pool_alloc(ctx, 2 * perm_words * 4, &S.perms))) break;
            uint32_t *pd = static_cast<uint32_t *>(S.perms);
            if ((rc = copy_h2d_bounced(ctx, pd, perms1, perm_words * 4, ctx->s_commit))) break;
            if ((rc = copy_h2d_bounced(ctx, pd + perm_words, perms2, perm_words * 4, ctx->s_commit))) break;
        }
        // the launch of commit_impl for `total` rows: as many workgroups as stay resident, equal chunks of about four
        // rounds (a chunk end is where the kernel builds the upper tree levels of the rows it has finished)
        const CommitGeom geom = commit_geom(cw, C);
        uint32_t G = ctx->num_cus * commit_wgs_per_cu(geom);
        if (G > total) G = total;
        const uint32_t rounds = (total + G - 1) / G;
        uint32_t nch = rounds >= 8 ? std::min(8u, rounds / 4) : rounds >= 2 ? 2u : 1u;
        const uint32_t rpc = (rounds + nch - 1) / nch;
        CommitArgs a{};
        a.classes = 1;
        a.evals = b->evals_d;
        a.perm1 = codes ? static_cast<const uint32_t *>(S.perms) : ctx->perm1_d;
        a.perm2 = codes ? static_cast<const uint32_t *>(S.perms) + perm_words : ctx->perm2_d;
        a.log_member_rows = ilog2(R);
        a.rows = static_cast<uint64_t *>(S.rows);
        a.compact_rows = 1u;
        a.layers = static_cast<uint32_t *>(S.layers);
        a.row_len = C;
        a.cw = cw;
        a.num_rows = total;
        a.rounds_per_chunk = rpc;
        a.roots = static_cast<uint32_t *>(S.roots);
        if ((rc = codes ? dispatch_commit_codes(ctx, a, G, ctx->s_commit) : dispatch_commit<true>(ctx, a, G, ctx->s_commit))) break;
        // the handle and its members are complete when this call returns: nothing later has to wait for the commit
        hipError_t e = stream_wait(ctx->s_commit);
        if (e != hipSuccess) { rc = fail(ctx, ZIP_ERR_HIP, "batch commit failed: %s", hipGetErrorString(e)); break; }
        if (roots_out && (rc = copy_d2h_bounced(ctx, roots_out, S.roots, (size_t)total * 32, ctx->stream))) break;
    } while (0);
    if (rc) {
        delete b;
        return rc;
    }
    *out = b;
    return ZIP_OK;
}

int32_t zip_batch_commit(zip_ctx *ctx, const int64_t *evals, size_t n_evals, uint32_t n_polys, zip_mem_kind evals_kind,
                         uint8_t *roots_out, zip_batch **out) {
    return batch_commit_impl(ctx, evals, n_evals, n_polys, evals_kind, false, nullptr, nullptr, roots_out, out);
}

int32_t zip_batch_commit_codes(zip_ctx *ctx, const int64_t *evals, size_t n_evals, uint32_t n_polys, zip_mem_kind evals_kind,
                               const uint32_t *perms1, const uint32_t *perms2, uint8_t *roots_out, zip_batch **out) {
    return batch_commit_impl(ctx, evals, n_evals, n_polys, evals_kind, true, perms1, perms2, roots_out, out);
}

void zip_batch_codes_counts(uint64_t *commits, uint64_t *members, uint64_t *field_opens) {
    if (commits) *commits = g_batch_codes_commits.load();
    if (members) *members = g_batch_codes_members.load();
    if (field_opens) *field_opens = g_batch_field_opens.load();
}

uint32_t zip_batch_size(const zip_batch *b) { return b ? b->n_polys : 0; }

void zip_batch_free(zip_batch *b) {
    if (!b) return;
    std::lock_guard<std::recursive_mutex> api_lock(b->ctx->api_mu);
    delete b;  // (the storage goes with the last of the batch and its members)
}

int32_t zip_batch_member(zip_batch *b, uint32_t index, zip_commitment **out) {
    if (!b || !out) return ZIP_ERR_NULL;
    *out = nullptr;
    zip_ctx *ctx = b->ctx;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (index >= b->n_polys)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "member %u of a batch of %u polynomials", index, b->n_polys);
    zip_commitment *c = new (std::nothrow) zip_commitment();
    if (!c) return ZIP_ERR_ALLOC;
    const size_t R = ctx->p.num_rows, C = ctx->p.row_len, cw = ctx->p.codeword_len;
    c->ctx = ctx;
    c->store = b->store;
    c->borrows_rows = c->borrows_rest = true;
    c->compact_rows = true;
    c->rows_bytes = R * cw * 16;
    c->layers_bytes = R * 2 * cw * 32;
    c->roots_bytes = R * 32;
    c->evals_bytes = R * C * 8;
    c->rows = static_cast<uint64_t *>(b->store->rows) + (size_t)index * R * cw * 2;
    c->layers = static_cast<uint32_t *>(b->store->layers) + (size_t)index * R * 2 * cw * 8;
    c->roots = static_cast<uint32_t *>(b->store->roots) + (size_t)index * R * 8;
    c->evals = const_cast<int64_t *>(b->evals_d) + (size_t)index * R * C;  // (only ever read)
    *out = c;
    return ZIP_OK;
}

// The fields of a _fields call: FieldConfig::new per member, before anything reaches the device.  Every NULL first, then
// the limb counts (one for all, 2 .. 4), then the moduli (odd, above 1); neighbours with the same modulus share the work.
static int32_t batch_member_fields(zip_ctx *ctx, const zip_field *const *fields, uint32_t B, std::vector<HostField> *out) {
    if (!fields) return fail(ctx, ZIP_ERR_NULL, "fields is NULL");
    for (uint32_t i = 0; i < B; i++)
        if (!fields[i]) return fail(ctx, ZIP_ERR_NULL, "fields[%u] is NULL", i);
    const uint32_t fl = fields[0]->limbs;
    if (fl < 2 || fl > 4) return fail(ctx, ZIP_ERR_INVALID_PARAM, "field limbs %u not in {2,3,4}", fl);
    for (uint32_t i = 1; i < B; i++)
        if (fields[i]->limbs != fl)
            return fail(ctx, ZIP_ERR_INVALID_PARAM, "member %u: a field of %u limbs, member 0 has %u", i, fields[i]->limbs, fl);
    out->resize(B);
    for (uint32_t i = 0; i < B; i++) {
        if (i && !memcmp(fields[i]->modulus, fields[i - 1]->modulus, 8 * (size_t)fl)) {
            (*out)[i] = (*out)[i - 1];
            continue;
        }
        if (int32_t rc = make_field_uncached(ctx, fields[i], &(*out)[i])) return rc;
    }
    return ZIP_OK;
}

// The one-field calls (fields == nullptr) and the _fields calls (field == nullptr) share everything but the field checks
// -- the latter's run before the device is touched -- and the row combination's kernel.
static int32_t batch_open_eval_impl(zip_batch *b, const uint64_t *q0_mont, const zip_field *field, const zip_field *const *fields,
                                    bool per_member, uint64_t *rows_out, zip_mem_kind out_kind) {
    if (!b || !rows_out) return ZIP_ERR_NULL;
    zip_ctx *ctx = b->ctx;
    if (!per_member) HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    HostField hf;
    std::vector<HostField> hfs;
    int32_t rc;
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, B = b->n_polys;
    if (per_member) {
        if ((rc = batch_member_fields(ctx, fields, B, &hfs))) return rc;
        hf = hfs[0];
    } else if ((rc = make_field(ctx, field, &hf))) return rc;
    const bool single = R == 1;
    if (!single && !q0_mont) return fail(ctx, ZIP_ERR_NULL, "q0_mont is NULL");
    std::vector<unsigned char> inst_h;
    std::vector<uint64_t> ones_h;
    if (per_member) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        g_batch_field_opens++;
        with_fl(hf.fl, [&](auto FL) { batch_fill_field_args<decltype(FL)::value>(hfs, &inst_h, &ones_h); });
    }
    const size_t bytes = (size_t)B * C * hf.fl * 8;
    Scratch res(ctx), small(ctx);
    uint64_t *out_d = rows_out;
    if (out_kind == ZIP_MEM_HOST) {
        if ((rc = res.get(bytes))) return rc;
        out_d = res.as<uint64_t>();
    }
    SmallInputs si;
    // one row: the evaluation row is map_to_field(evals) = 1_mont * w (open_z.rs:84-88), 1_mont of the member's field
    si.src[1] = !single ? (const void *)q0_mont : per_member ? (const void *)ones_h.data() : (const void *)hf.r;
    si.bytes[1] = single && !per_member ? (size_t)hf.fl * 8 : (size_t)B * R * hf.fl * 8;
    si.src[3] = inst_h.data();
    si.bytes[3] = inst_h.size();
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    BatchCombineArgs a{};
    a.evals = b->evals_d;
    a.q0 = reinterpret_cast<const uint64_t *>(sb + si.off[1]);
    a.q0_shared = single && !per_member ? 1u : 0u;
    a.num_rows = R;
    a.row_len = C;
    a.m_limbs = ctx->p.m_limbs;
    a.quirk_mod = hf.quirk_mod;
    a.row_limbs = out_d;
    if (per_member)
        rc = with_fl(hf.fl, [&](auto FL) { return launch_batch_combine_fields_fl<decltype(FL)::value>(ctx, a, B, false, sb + si.off[3]); });
    else rc = launch_batch_combine(ctx, a, B, false, hf);
    if (rc) return rc;
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, rows_out, ZIP_MEM_HOST, out_d, bytes);
    HIP_TRY(ctx, stream_wait(ctx->stream));  // q0 was read from host memory
    return ZIP_OK;
}

int32_t zip_batch_open_eval(zip_batch *b, const uint64_t *q0_mont, const zip_field *field, uint64_t *rows_out,
                            zip_mem_kind out_kind) {
    return batch_open_eval_impl(b, q0_mont, field, nullptr, false, rows_out, out_kind);
}

int32_t zip_batch_open_eval_fields(zip_batch *b, const uint64_t *q0_mont, const zip_field *const *fields, uint64_t *rows_out,
                                   zip_mem_kind out_kind) {
    return batch_open_eval_impl(b, q0_mont, nullptr, fields, true, rows_out, out_kind);
}

static int32_t batch_open_impl(zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont,
                               const zip_field *field, const zip_field *const *fields, bool per_member, uint8_t *proofs_out,
                               zip_mem_kind out_kind) {
    if (!b || !proofs_out || (n_cols && !cols)) return ZIP_ERR_NULL;
    zip_ctx *ctx = b->ctx;
    if (!per_member) HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    HostField hf;
    std::vector<HostField> hfs;
    int32_t rc;
    if ((rc = refuse_extra_tests(ctx, per_member ? "zip_batch_open_fields" : "zip_batch_open"))) return rc;
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, B = b->n_polys;
    if (per_member) {
        if ((rc = batch_member_fields(ctx, fields, B, &hfs))) return rc;
        hf = hfs[0];
    } else if ((rc = make_field(ctx, field, &hf))) return rc;
    const bool single = R == 1;
    if (!single && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if ((uint64_t)B * n_cols > 0xFFFFFFFFull) return fail(ctx, ZIP_ERR_UNSUPPORTED, "%u x %u openings exceed 2^32", B, n_cols);
    if ((rc = check_cols(ctx, cols, B * n_cols))) return rc;
    std::vector<unsigned char> inst_h;
    std::vector<uint64_t> ones_h;
    if (per_member) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        g_batch_field_opens++;
        with_fl(hf.fl, [&](auto FL) { batch_fill_field_args<decltype(FL)::value>(hfs, &inst_h, &ones_h); });
    }
    const size_t stream_bytes = zip_proof_len(ctx, n_cols, hf.fl), total = (size_t)B * stream_bytes;
    const size_t u_bytes = single ? 0 : (size_t)C * ctx->p.m_limbs * 8;
    const size_t col_bytes = (size_t)n_cols * column_bytes(ctx);
    Scratch res(ctx), small(ctx);
    uint8_t *out_d = proofs_out;
    if (out_kind == ZIP_MEM_HOST) {
        if ((rc = res.get(total))) return rc;
        out_d = res.as<uint8_t>();
    }
    SmallInputs si;
    if (!single) {
        si.src[0] = coeffs;
        si.bytes[0] = (size_t)B * R * 8;
    }
    si.src[1] = !single ? (const void *)q0_mont : per_member ? (const void *)ones_h.data() : (const void *)hf.r;
    si.bytes[1] = single && !per_member ? (size_t)hf.fl * 8 : (size_t)B * R * hf.fl * 8;
    si.src[2] = cols;
    si.bytes[2] = (size_t)B * n_cols * 4;
    si.src[3] = inst_h.data();
    si.bytes[3] = inst_h.size();
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    // 1. every polynomial's u' and evaluation row, straight to their places in its stream
    BatchCombineArgs a{};
    a.evals = b->evals_d;
    a.coeffs = single ? nullptr : reinterpret_cast<const int64_t *>(sb + si.off[0]);
    a.q0 = reinterpret_cast<const uint64_t *>(sb + si.off[1]);
    a.q0_shared = single && !per_member ? 1u : 0u;
    a.num_rows = R;
    a.row_len = C;
    a.m_limbs = ctx->p.m_limbs;
    a.quirk_mod = hf.quirk_mod;
    a.uprime = single ? nullptr : out_d;
    a.row_be = out_d + u_bytes + col_bytes;
    a.out_stride = stream_bytes;
    if (per_member)
        rc = with_fl(hf.fl, [&](auto FL) { return launch_batch_combine_fields_fl<decltype(FL)::value>(ctx, a, B, !single, sb + si.off[3]); });
    else rc = launch_batch_combine(ctx, a, B, !single, hf);
    if (rc) return rc;
    // 2. every polynomial's column openings
    if (n_cols) {
        BatchOpenColsArgs g{};
        g.rows = static_cast<const uint64_t *>(b->store->rows);
        g.layers = static_cast<const uint64_t *>(b->store->layers);
        g.cols = reinterpret_cast<const uint32_t *>(sb + si.off[2]);
        g.out = out_d;
        g.stream_bytes = stream_bytes;
        g.openings_at = u_bytes;
        g.n_cols = n_cols;
        g.num_rows = R;
        g.cw = ctx->p.codeword_len;
        g.depth = ctx->depth;
        g.rows_per_block = R < 32u ? R : 32u;
        // (cw <= 16384: 2 * depth + 1 <= 29 lanes per row; an image of 32 records is at most 14.6 KB)
        const size_t lds = (size_t)g.rows_per_block * (8 + 32 * (size_t)ctx->depth);
        const dim3 grid(n_cols, (R + g.rows_per_block - 1) / g.rows_per_block, B), block(256);
        LaunchTimer t(ctx, "batch_open_columns_kernel", ctx->stream);
        hipLaunchKernelGGL(batch_open_columns_kernel<32>, grid, block, lds, ctx->stream, g);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (out_kind == ZIP_MEM_HOST) return deliver(ctx, proofs_out, ZIP_MEM_HOST, out_d, total);
    HIP_TRY(ctx, stream_wait(ctx->stream));  // coeffs, cols and q0 were read from host memory
    return ZIP_OK;
}

int32_t zip_batch_open(zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont,
                       const zip_field *field, uint8_t *proofs_out, zip_mem_kind out_kind) {
    return batch_open_impl(b, coeffs, cols, n_cols, q0_mont, field, nullptr, false, proofs_out, out_kind);
}

int32_t zip_batch_open_fields(zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont,
                              const zip_field *const *fields, uint8_t *proofs_out, zip_mem_kind out_kind) {
    return batch_open_impl(b, coeffs, cols, n_cols, q0_mont, nullptr, fields, true, proofs_out, out_kind);
}

// ---- zip_batch_open_each: zip_batch_open_fields with every stream delivered to a destination of its own ----
// HOST destinations: the members leave in windows of W; two staging slots of W streams, the gather of window w + 1 on
// ctx->stream beside the copies of window w on s_upper (zip_open_stream's pattern).  DEVICE destinations: one launch
// pair that writes through a device table of the destinations, no staging.
// Process-wide (zip_batch_open_each_counts): calls that reached the device, their members and windows, and the staging
// bytes of the last of them
static std::atomic<uint64_t> g_open_each_calls{0}, g_open_each_members{0}, g_open_each_windows{0}, g_open_each_staging{0};

int32_t zip_batch_open_each(zip_batch *b, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont,
                            const zip_field *const *fields, uint8_t *const *proofs_out, zip_mem_kind out_kind, size_t window_bytes) {
    if (!b || !proofs_out || (n_cols && !cols)) return ZIP_ERR_NULL;
    zip_ctx *ctx = b->ctx;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, B = b->n_polys;
    for (uint32_t i = 0; i < B; i++)
        if (!proofs_out[i]) return fail(ctx, ZIP_ERR_NULL, "proofs_out[%u] is NULL", i);
    std::vector<HostField> hfs;
    int32_t rc;
    if ((rc = refuse_extra_tests(ctx, "zip_batch_open_each"))) return rc;
    if ((rc = batch_member_fields(ctx, fields, B, &hfs))) return rc;
    const HostField &hf = hfs[0];
    const bool single = R == 1;
    if (!single && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if ((uint64_t)B * n_cols > 0xFFFFFFFFull) return fail(ctx, ZIP_ERR_UNSUPPORTED, "%u x %u openings exceed 2^32", B, n_cols);
    if ((rc = check_cols(ctx, cols, B * n_cols))) return rc;
    const size_t len = zip_proof_len(ctx, n_cols, hf.fl);
    {   // the destinations: aligned for the kernels' stores where they write them, and disjoint
        std::vector<uintptr_t> at(B);
        for (uint32_t i = 0; i < B; i++) {
            at[i] = reinterpret_cast<uintptr_t>(proofs_out[i]);
            if (out_kind == ZIP_MEM_DEVICE && (at[i] & 7))
                return fail(ctx, ZIP_ERR_INVALID_PARAM, "proofs_out[%u] is a device address that is not 8-byte aligned", i);
        }
        std::sort(at.begin(), at.end());
        for (uint32_t i = 1; i < B; i++)
            if (at[i] - at[i - 1] < len) return fail(ctx, ZIP_ERR_INVALID_PARAM, "two destinations of %zu bytes overlap", len);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool to_host = out_kind == ZIP_MEM_HOST;
    if (window_bytes == 0) window_bytes = (size_t)64 << 20;
    const uint32_t W = to_host ? (uint32_t)std::min<size_t>(std::max<size_t>(window_bytes / len, 1), B) : B;
    const uint32_t n_windows = (B + W - 1) / W, n_slots = !to_host ? 0u : n_windows > 1 ? 2u : 1u;
    std::vector<unsigned char> inst_h;
    std::vector<uint64_t> ones_h;
    with_fl(hf.fl, [&](auto FL) { batch_fill_field_args<decltype(FL)::value>(hfs, &inst_h, &ones_h); });
    const size_t u_bytes = single ? 0 : (size_t)C * ctx->p.m_limbs * 8;
    const size_t col_bytes = (size_t)n_cols * column_bytes(ctx);
    Scratch slot0(ctx), slot1(ctx), small(ctx);
    if (n_slots > 0 && (rc = slot0.get((size_t)W * len))) return rc;
    if (n_slots > 1 && (rc = slot1.get((size_t)W * len))) return rc;
    uint8_t *slot[2] = {slot0.as<uint8_t>(), slot1.as<uint8_t>()};
    SmallInputs si;
    if (!single) {
        si.src[0] = coeffs;
        si.bytes[0] = (size_t)B * R * 8;
    }
    si.src[1] = single ? (const void *)ones_h.data() : (const void *)q0_mont;
    si.bytes[1] = (size_t)B * R * hf.fl * 8;
    si.src[2] = cols;
    si.bytes[2] = (size_t)B * n_cols * 4;
    si.src[3] = inst_h.data();
    si.bytes[3] = inst_h.size();
    if (!to_host) {
        si.src[4] = proofs_out;
        si.bytes[4] = (size_t)B * sizeof(uint8_t *);
    }
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    // the inputs are on their way: from here on the call has reached the device
    g_batch_field_opens++;
    g_open_each_calls++;
    g_open_each_members += B;
    g_open_each_windows += n_windows;
    g_open_each_staging = (uint64_t)n_slots * W * len;
    BatchCombineArgs a{};
    a.evals = b->evals_d;
    a.coeffs = single ? nullptr : reinterpret_cast<const int64_t *>(sb + si.off[0]);
    a.q0 = reinterpret_cast<const uint64_t *>(sb + si.off[1]);
    a.num_rows = R;
    a.row_len = C;
    a.m_limbs = ctx->p.m_limbs;
    a.out_stride = len;
    BatchOpenColsArgs g{};
    g.rows = static_cast<const uint64_t *>(b->store->rows);
    g.layers = static_cast<const uint64_t *>(b->store->layers);
    g.cols = reinterpret_cast<const uint32_t *>(sb + si.off[2]);
    g.stream_bytes = len;
    g.openings_at = u_bytes;
    g.n_cols = n_cols;
    g.num_rows = R;
    g.cw = ctx->p.codeword_len;
    g.depth = ctx->depth;
    g.rows_per_block = R < 32u ? R : 32u;
    // members [first, first + cnt): u' and the evaluation row, then the column openings, to `out` (a slot) or the table
    auto launch = [&](uint32_t first, uint32_t cnt, uint8_t *out) -> int32_t {
        BatchEachArgs e{};
        e.first = first;
        if (out) {
            a.uprime = single ? nullptr : out;
            a.row_be = out + u_bytes + col_bytes;
        } else {
            e.dst = reinterpret_cast<uint8_t *const *>(sb + si.off[4]);
            e.row_be_at = u_bytes + col_bytes;
        }
        int32_t r = with_fl(hf.fl, [&](auto FL) {
            return launch_batch_combine_each_fl<decltype(FL)::value>(ctx, a, cnt, !single, sb + si.off[3], e);
        });
        if (r || !n_cols) return r;
        g.out = out;
        return launch_batch_open_columns_each(ctx, g, cnt, e);
    };
    if (!to_host) {
        if ((rc = launch(0, B, nullptr))) return rc;
        HIP_TRY(ctx, stream_wait(ctx->stream));  // coeffs, cols, q0 and the table were read from host memory
        return ZIP_OK;
    }
    hipStream_t s_copy = ctx->s_upper;  // the copies of window w run beside the gather of window w + 1
    hipEvent_t gathered[2] = {take_dep_event(ctx), take_dep_event(ctx)};
    hipEvent_t copied[2] = {take_dep_event(ctx), take_dep_event(ctx)};
    auto launch_window = [&](uint32_t w) -> int32_t {
        const int s = (int)(w & 1);
        const uint32_t first = w * W;
        if (w >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, copied[s], 0));  // slot[s] has left the device
        if (int32_t r = launch(first, std::min(W, B - first), slot[s])) return r;
        HIP_TRY(ctx, hipEventRecord(gathered[s], ctx->stream));
        return ZIP_OK;
    };
    auto copy_window = [&](uint32_t w) -> int32_t {
        const int s = (int)(w & 1);
        const uint32_t first = w * W, cnt = std::min(W, B - first);
        for (uint32_t i = 0; i < cnt; i++) {
            uint8_t *dst = proofs_out[first + i];
            const uint8_t *src = slot[s] + (size_t)i * len;
            if (host_range_is_pinned(dst, len)) HIP_TRY(ctx, hipMemcpyAsync(dst, src, len, hipMemcpyDeviceToHost, s_copy));
            else if (int32_t r = copy_d2h_bounced(ctx, dst, src, len, s_copy)) return r;
        }
        HIP_TRY(ctx, hipEventRecord(copied[s], s_copy));
        return ZIP_OK;
    };
    int32_t status = launch_window(0);
    for (uint32_t w = 0; w < n_windows && status == ZIP_OK; w++) {
        hipError_t e = hipStreamWaitEvent(s_copy, gathered[w & 1], 0);
        if (e != hipSuccess) { status = fail(ctx, ZIP_ERR_HIP, "hipStreamWaitEvent: %s", hipGetErrorString(e)); break; }
        if (w + 1 < n_windows && (status = launch_window(w + 1))) break;
        status = copy_window(w);
    }
    // every byte has landed, and nothing still reads the slots, before they return to the pool
    hipError_t e1 = stream_wait(s_copy), e2 = stream_wait(ctx->stream);
    for (int i = 0; i < 2; i++) {
        ctx->dep_event_pool.push_back(gathered[i]);
        ctx->dep_event_pool.push_back(copied[i]);
    }
    if (status) return status;
    HIP_TRY(ctx, e1);
    HIP_TRY(ctx, e2);
    return ZIP_OK;
}

void zip_batch_open_each_counts(uint64_t *calls, uint64_t *members, uint64_t *windows, uint64_t *last_staging_bytes) {
    if (calls) *calls = g_open_each_calls.load();
    if (members) *members = g_open_each_members.load();
    if (windows) *windows = g_open_each_windows.load();
    if (last_staging_bytes) *last_staging_bytes = g_open_each_staging.load();
}

// =====================================================================================================
// Several GPUs behind ONE call (single process as the reference's callers are:
// src/zinc/prover.rs:305-328, benches/zip_benches.rs:100-168).  A zip_mctx owns one row-shard zip_ctx per entry
// of `devices` (an ordinal may repeat: several shards on one GPU, which is how this is tested on a one-GPU box).
// Rows are independent until the very end (commit.rs:71-74,172-178), so a commit + open is
//   per shard   hinted persistent commit of its rows -> roots slice; fused row combinations over its rows
//               (partial u', partial evaluation row, exact: integer / modular sums are associative); the
//               openings of ITS rows of every column, pipelined behind its own commit kernel
//   lead shard  sum of the partial rows (the one exchange besides the 32-byte roots: 96 bytes per column and shard)
// and the proof stream is assembled where it is wanted: in host memory every shard delivers its row slice of
// every column over its OWN PCIe link (two pitched copies), which is the point of sharding a path whose
// single-GPU cost is dominated by moving 1.74 GiB to the host.
// =====================================================================================================
struct zip_mctx {
    std::vector<zip_ctx *> shard;
    std::vector<int64_t *> witness;      // per shard: its rows of the witness (device), or null
    std::vector<uint8_t *> slice;        // per shard: [n_cols][count * 32 | count * rec] openings of its rows
    std::vector<size_t> slice_bytes;
    std::vector<uint64_t *> upart, fpart;  // per shard: partial u' [row_len][m_limbs], partial row [row_len][fl]
    std::vector<hipEvent_t> combined;
    uint64_t *uparts_all = nullptr, *fparts_all = nullptr;  // lead device: [G][...]
    uint8_t *ends = nullptr;             // lead device: u' (row_len * 64) | evaluation row big-endian (row_len * 8 fl)
    size_t ends_cap = 0;
    uint32_t last_cols = 0, last_fl = 0;
    // the one exchange of the commit (commit.rs:78-81): every shard's roots on EVERY device, [num_rows][32].
    // Distinct devices: an in-process RCCL communicator per shard (ncclCommInitAll) and one grouped all-gather over
    // xGMI; repeated ordinals (several shards on one GPU: the one-GPU rehearsal) or no librccl: device copies.
    std::vector<uint8_t *> roots_all;
    std::vector<void *> nccl_comm;  // ncclComm_t per shard, or empty
    std::string roots_path = "none";
    std::string last_error;
    std::mutex mu;
};

// librccl is bound at run time (dlopen), only by a zip_mctx over several distinct devices: libzip_hip.so itself has no
// RCCL dependency, and a process that already carries an RCCL (PyTorch's) gets that copy.
namespace rccl {
// (the function-pointer types: rccl_dyn.h -- RCCL's own prototypes where its header exists)
struct Api {
    void *lib = nullptr;
    comm_init_all_t comm_init_all = nullptr;
    comm_destroy_t comm_destroy = nullptr;
    group_t group_start = nullptr, group_end = nullptr;
    all_gather_t all_gather = nullptr;
    broadcast_t broadcast = nullptr;
    err_str_t err_str = nullptr;
    bool ok = false;
};
static Api &api() {
    static Api a;
    static std::once_flag once;
    std::call_once(once, [] {
        if (getenv("ZIP_HIP_NO_RCCL")) return;  // (per process; per zip_mctx: ZIP_HIP_MCTX_FORCE_NO_RCCL, zip_mctx_create)
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (!a.lib) return;
        a.comm_init_all = (comm_init_all_t)dlsym(a.lib, "ncclCommInitAll");
        a.comm_destroy = (comm_destroy_t)dlsym(a.lib, "ncclCommDestroy");
        a.group_start = (group_t)dlsym(a.lib, "ncclGroupStart");
        a.group_end = (group_t)dlsym(a.lib, "ncclGroupEnd");
        a.all_gather = (all_gather_t)dlsym(a.lib, "ncclAllGather");
        a.broadcast = (broadcast_t)dlsym(a.lib, "ncclBroadcast");
        a.err_str = (err_str_t)dlsym(a.lib, "ncclGetErrorString");
        a.ok = a.comm_init_all && a.comm_destroy && a.group_start && a.group_end && a.all_gather && a.broadcast;
    });
    return a;
}
}  // namespace rccl

static int32_t mfail(zip_mctx *m, int32_t code, const char *what, zip_ctx *from = nullptr) {
    m->last_error = std::string(what) + (from ? std::string(": ") + from->last_error : std::string());
    return code;
}

const char *zip_mctx_last_error(const zip_mctx *m) { return m ? m->last_error.c_str() : ""; }
uint32_t zip_mctx_shards(const zip_mctx *m) { return m ? (uint32_t)m->shard.size() : 0; }
zip_ctx *zip_mctx_shard_ctx(zip_mctx *m, uint32_t s) { return (m && s < m->shard.size()) ? m->shard[s] : nullptr; }

void zip_mctx_destroy(zip_mctx *m) {
    if (!m) return;
    for (size_t s = 0; s < m->shard.size(); s++) {
        zip_ctx *ctx = m->shard[s];
        if (!ctx) continue;
        (void)hipSetDevice(ctx->device);
        (void)zip_ctx_synchronize(ctx);
        if (s < m->witness.size()) pool_release(ctx, m->witness[s]);
        if (s < m->slice.size()) pool_release(ctx, m->slice[s]);
        if (s < m->upart.size()) pool_release(ctx, m->upart[s]);
        if (s < m->fpart.size()) pool_release(ctx, m->fpart[s]);
        if (s < m->combined.size() && m->combined[s]) (void)hipEventDestroy(m->combined[s]);
        if (s < m->roots_all.size()) pool_release(ctx, m->roots_all[s]);
        if (s == 0) {
            pool_release(ctx, m->uparts_all);
            pool_release(ctx, m->fparts_all);
            pool_release(ctx, m->ends);
        }
    }
    for (void *c : m->nccl_comm)
        if (c && rccl::api().ok) (void)rccl::api().comm_destroy(static_cast<rccl::comm_t>(c));
    for (zip_ctx *ctx : m->shard) zip_ctx_destroy(ctx);
    delete m;
}

int32_t zip_mctx_create(const zip_params *p, int32_t n_devices, const int32_t *devices, zip_mctx **out) {
    if (!p || !out || !devices) return ZIP_ERR_NULL;
    *out = nullptr;
    if (p->n_limbs == 2 && p->k_limbs == 8 && p->m_limbs == 16) return ZIP_ERR_UNSUPPORTED;  // a two-limb ctx has no row shards
    if (n_devices < 1 || (uint32_t)n_devices > p->num_rows || n_devices > 64) return ZIP_ERR_INVALID_PARAM;
    zip_mctx *m = new (std::nothrow) zip_mctx();
    if (!m) return ZIP_ERR_ALLOC;
    const uint32_t G = (uint32_t)n_devices, R = p->num_rows;
    int32_t rc = ZIP_OK;
    for (uint32_t s = 0; s < G && !rc; s++) {
        zip_params ps = *p;
        ps.device = devices[s];
        ps.row_begin = (uint32_t)((uint64_t)R * s / G);  // contiguous blocks of rows, as even as they come
        ps.row_count = (uint32_t)((uint64_t)R * (s + 1) / G) - ps.row_begin;
        zip_ctx *ctx = nullptr;
        rc = zip_ctx_create(&ps, &ctx);
        m->shard.push_back(ctx);
    }
    if (!rc) {
        m->witness.assign(G, nullptr);
        m->slice.assign(G, nullptr);
        m->slice_bytes.assign(G, 0);
        m->upart.assign(G, nullptr);
        m->fpart.assign(G, nullptr);
        m->combined.assign(G, nullptr);
        for (uint32_t s = 0; s < G && !rc; s++) {
            if (hipSetDevice(m->shard[s]->device) != hipSuccess ||
                hipEventCreateWithFlags(&m->combined[s], hipEventDisableTiming) != hipSuccess)
                rc = ZIP_ERR_HIP;
            // the lead device pulls every shard's partial rows: peer access where the devices differ
            if (!rc && s > 0 && m->shard[s]->device != m->shard[0]->device) {
                int can = 0;
                (void)hipSetDevice(m->shard[0]->device);
                // (ZIP_HIP_MCTX_FORCE_NO_PEER=1: as on a box whose devices cannot map each other -- hipMemcpyPeerAsync
                // then stages through the host; same bytes)
                if (!getenv("ZIP_HIP_MCTX_FORCE_NO_PEER") && hipDeviceCanAccessPeer(&can, m->shard[0]->device, m->shard[s]->device) == hipSuccess && can) {
                    hipError_t e = hipDeviceEnablePeerAccess(m->shard[s]->device, 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) rc = ZIP_ERR_HIP;
                    (void)hipGetLastError();
                }
            }
        }
    }
    if (!rc) {
        m->roots_all.assign(G, nullptr);
        bool distinct = true;
        for (uint32_t s = 0; s < G; s++)
            for (uint32_t t = 0; t < s; t++) distinct &= devices[s] != devices[t];
        // (ZIP_HIP_MCTX_FORCE_NO_RCCL=1: as on a box without a usable librccl -- the roots travel as device copies)
        if (distinct && !getenv("ZIP_HIP_MCTX_FORCE_NO_RCCL") && rccl::api().ok) {
            m->nccl_comm.assign(G, nullptr);
            std::vector<int> devs(devices, devices + G);
            std::vector<rccl::comm_t> comms(G, nullptr);
            const int e = (int)rccl::api().comm_init_all(comms.data(), (int)G, devs.data());
            for (uint32_t s = 0; s < G; s++) m->nccl_comm[s] = comms[s];
            if (e != 0) {  // (not fatal: the roots then travel as peer copies; zip_mctx_roots_path says which)
                m->last_error = std::string("ncclCommInitAll failed: ") + (rccl::api().err_str ? rccl::api().err_str((rccl::result_t)e) : "?");
                m->nccl_comm.clear();
            }
        }
    }
    if (rc) {
        zip_mctx_destroy(m);
        return rc;
    }
    *out = m;
    return ZIP_OK;
}

// The commitment of the last zip_mctx_commit_open as every device holds it: the roots of ALL rows, [num_rows][32], on
// shard s's device (valid until the next call on m).
int32_t zip_mctx_roots(zip_mctx *m, uint32_t s, uint8_t **ptr) {
    if (!m || !ptr || s >= m->shard.size()) return ZIP_ERR_NULL;
    *ptr = s < m->roots_all.size() ? m->roots_all[s] : nullptr;
    return *ptr ? ZIP_OK : ZIP_ERR_INVALID_PARAM;
}
// "rccl" (grouped ncclAllGather / ncclBroadcast over the in-process communicators), "copies" (device copies: repeated
// ordinals, or librccl missing / refused) or "none" (no zip_mctx_commit_open yet)
const char *zip_mctx_roots_path(const zip_mctx *m) { return m ? m->roots_path.c_str() : ""; }

// Places the witness on the devices: shard s gets its rows.  evals: HOST, the whole polynomial.
int32_t zip_mctx_set_witness(zip_mctx *m, const int64_t *evals, size_t n_evals) {
    if (!m || !evals) return ZIP_ERR_NULL;
    std::lock_guard<std::mutex> g(m->mu);
    const zip_ctx *c0 = m->shard[0];
    if (n_evals != (size_t)c0->p.num_rows * c0->p.row_len)
        return mfail(m, ZIP_ERR_SHAPE, "Polynomial has an incorrect number of evaluations for the expected matrix size");
    for (size_t s = 0; s < m->shard.size(); s++) {
        zip_ctx *ctx = m->shard[s];
        if (hipSetDevice(ctx->device) != hipSuccess) return mfail(m, ZIP_ERR_HIP, "hipSetDevice failed");
        const size_t n = (size_t)ctx->rows_local * ctx->p.row_len;
        int32_t rc;
        if (!m->witness[s] && (rc = pool_alloc(ctx, n * 8, (void **)&m->witness[s]))) return mfail(m, rc, "witness slice", ctx);
        if ((rc = copy_h2d_bounced(ctx, m->witness[s], evals + (size_t)ctx->p.row_begin * ctx->p.row_len, n * 8, ctx->stream)))
            return mfail(m, rc, "witness upload", ctx);
        if (stream_wait(ctx->stream) != hipSuccess) return mfail(m, ZIP_ERR_HIP, "witness upload failed");
    }
    return ZIP_OK;
}

// Device address and size of shard s's openings after zip_mctx_commit_open: [n_cols][count * 32 bytes of values |
// count records], its rows of every opened column in wire format (valid until the next call).
int32_t zip_mctx_shard_openings(zip_mctx *m, uint32_t s, uint8_t **ptr, size_t *bytes, uint32_t *row_begin, uint32_t *row_count) {
    if (!m || s >= m->shard.size()) return ZIP_ERR_NULL;
    if (ptr) *ptr = m->slice[s];
    if (bytes) *bytes = (size_t)m->last_cols * column_bytes(m->shard[s]);
    if (row_begin) *row_begin = m->shard[s]->p.row_begin;
    if (row_count) *row_count = m->shard[s]->rows_local;
    return ZIP_OK;
}
// Device address (lead device) of u' (row_len * m_limbs * 8 bytes, absent when num_rows == 1) followed by the
// evaluation row (row_len * 8 fl bytes, big-endian Montgomery) of the last zip_mctx_commit_open.
int32_t zip_mctx_ends(zip_mctx *m, uint8_t **ptr, size_t *u_bytes, size_t *row_bytes) {
    if (!m) return ZIP_ERR_NULL;
    const zip_ctx *c0 = m->shard[0];
    if (ptr) *ptr = m->ends;
    if (u_bytes) *u_bytes = c0->p.num_rows > 1 ? (size_t)c0->p.row_len * c0->p.m_limbs * 8 : 0;
    if (row_bytes) *row_bytes = (size_t)c0->p.row_len * m->last_fl * 8;
    return ZIP_OK;
}

int32_t zip_mctx_commit_open(zip_mctx *m, const int64_t *evals, const int64_t *coeffs, const uint32_t *cols,
                             uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field, uint8_t *roots_out,
                             uint8_t *proof_out) {
    if (!m || (n_cols && !cols)) return ZIP_ERR_NULL;
    std::lock_guard<std::mutex> g(m->mu);
    const uint32_t G = (uint32_t)m->shard.size();
    zip_ctx *lead = m->shard[0];
    const uint32_t R = lead->p.num_rows, C = lead->p.row_len;
    const bool single = R == 1;
    HostField hf;
    int32_t rc;
    for (zip_ctx *sc : m->shard)  // (reachable through zip_mctx_shard_ctx on a one-shard mctx only)
        if ((rc = refuse_extra_tests(sc, "zip_mctx_commit_open"))) return mfail(m, rc, "proximity tests", sc);
    if ((rc = make_field(lead, field, &hf))) return mfail(m, rc, "field", lead);
    if (!single && (!coeffs || !q0_mont)) return mfail(m, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if ((rc = check_cols(lead, cols, n_cols))) return mfail(m, rc, "cols", lead);
    const uint32_t fl = hf.fl, ml = lead->p.m_limbs;
    const size_t u_bytes = single ? 0 : (size_t)C * ml * 8, row_bytes = (size_t)C * fl * 8;
    const size_t rec = 8 + 32 * (size_t)lead->depth, per_col = (size_t)R * (32 + rec);
    static const uint32_t none = 0;
    std::vector<zip_commitment *> com(G, nullptr);
    std::vector<std::unique_ptr<Scratch>> small;
    std::vector<std::unique_ptr<CombineScratch>> cscr;
    std::vector<const uint32_t *> cols_dv(G, nullptr);
    // every exit path: drain the shards, then free the commitments (the scratch objects go after that)
    auto finish = [&](int32_t code) {
        for (uint32_t s = 0; s < G; s++) {
            (void)hipSetDevice(m->shard[s]->device);
            (void)zip_ctx_synchronize(m->shard[s]);
            if (com[s]) zip_commitment_free(com[s]);
        }
        return code;
    };
    // ---- 0. a host witness goes up first, every shard's rows over its own link at the same time (one host thread
    //         per shard: the bounce-buffer copy blocks its caller).  A host-side zip_commit would wait for its whole
    //         commit kernel before returning -- one shard after the other.
    if (evals) {
        std::vector<int32_t> up(G, ZIP_OK);
        std::vector<std::thread> th;
        for (uint32_t s = 0; s < G; s++) {
            zip_ctx *ctx = m->shard[s];
            const size_t n = (size_t)ctx->rows_local * C;
            if (!m->witness[s]) {
                if (hipSetDevice(ctx->device) != hipSuccess || pool_alloc(ctx, n * 8, (void **)&m->witness[s])) {
                    up[s] = ZIP_ERR_ALLOC;
                    continue;
                }
            }
            th.emplace_back([=, &up]() {
                if (hipSetDevice(ctx->device) != hipSuccess) { up[s] = ZIP_ERR_HIP; return; }
                up[s] = copy_h2d_bounced(ctx, m->witness[s], evals + (size_t)ctx->p.row_begin * C, n * 8, ctx->stream);
                if (!up[s] && stream_wait(ctx->stream) != hipSuccess) up[s] = ZIP_ERR_HIP;
            });
        }
        for (auto &t : th) t.join();
        for (uint32_t s = 0; s < G; s++)
            if (up[s]) return finish(mfail(m, up[s], "witness upload", m->shard[s]));
    }
    // ---- 1. every shard: hinted commit of its rows (asynchronous), row combinations, openings of its rows
    for (uint32_t s = 0; s < G; s++) {
        zip_ctx *ctx = m->shard[s];
        if (hipSetDevice(ctx->device) != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, "hipSetDevice failed"));
        const uint32_t rows = ctx->rows_local, r0 = ctx->p.row_begin;
        const size_t n = (size_t)rows * C;
        const int64_t *ev = m->witness[s];
        if (!ev) return finish(mfail(m, ZIP_ERR_NULL, "evals is NULL and zip_mctx_set_witness was not called"));
        if ((rc = commit_impl(ctx, ev, n, ZIP_MEM_DEVICE, 1, cols ? cols : &none, n_cols, nullptr, &com[s])))
            return finish(mfail(m, rc, "commit", ctx));
        const int64_t *ev_d = com[s]->evals ? com[s]->evals : com[s]->evals_ref;
        const size_t need_slice = (size_t)n_cols * column_bytes(ctx);
        if (m->slice_bytes[s] < need_slice) {
            pool_release(ctx, m->slice[s]);
            m->slice[s] = nullptr;
            m->slice_bytes[s] = 0;
            if ((rc = pool_alloc(ctx, need_slice ? need_slice : 16, (void **)&m->slice[s]))) return finish(mfail(m, rc, "openings", ctx));
            m->slice_bytes[s] = need_slice;
        }
        if (!m->upart[s] && (rc = pool_alloc(ctx, (size_t)C * 8 * 8, (void **)&m->upart[s]))) return finish(mfail(m, rc, "partials", ctx));
        if (!m->fpart[s] && (rc = pool_alloc(ctx, (size_t)C * 8 * 8, (void **)&m->fpart[s]))) return finish(mfail(m, rc, "partials", ctx));
        small.emplace_back(new Scratch(ctx));
        cscr.emplace_back(new CombineScratch(ctx));
        SmallInputs si;
        if (!single) {
            si.src[0] = coeffs + r0;
            si.bytes[0] = (size_t)rows * 8;
        }
        si.src[1] = single ? hf.r : q0_mont + (size_t)r0 * fl;
        si.bytes[1] = (size_t)rows * fl * 8;
        si.src[2] = cols;
        si.bytes[2] = (size_t)n_cols * 4;
        unsigned char *sb;
        if ((rc = stage_small(ctx, si, *small.back(), &sb))) return finish(mfail(m, rc, "inputs", ctx));
        cols_dv[s] = reinterpret_cast<const uint32_t *>(sb + si.off[2]);
        CombineOut o{};
        o.uprime = single ? nullptr : m->upart[s];
        o.row_limbs = m->fpart[s];
        // the pass over the witness first (beside the commit's first chunk), the openings, the fold of the partial
        // sums last -- the order zip_open uses
        if ((rc = run_combine(ctx, ev_d, reinterpret_cast<const int64_t *>(sb + si.off[0]),
                              reinterpret_cast<const uint64_t *>(sb + si.off[1]), &hf, !single, true, o,
                              cscr.back().get(), 1)))
            return finish(mfail(m, rc, "combine", ctx));
        if ((rc = run_open_columns_pipelined(com[s], cols_dv[s], n_cols, m->slice[s]))) return finish(mfail(m, rc, "openings", ctx));
        if ((rc = run_combine(ctx, ev_d, reinterpret_cast<const int64_t *>(sb + si.off[0]),
                              reinterpret_cast<const uint64_t *>(sb + si.off[1]), &hf, !single, true, o,
                              cscr.back().get(), 2)))
            return finish(mfail(m, rc, "combine", ctx));
        if (hipEventRecord(m->combined[s], ctx->stream) != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, "event record failed"));
    }
    // ---- 1b. the roots of every shard onto every device (the commitment is device-resident everywhere), on the
    //          shards' commit streams: behind their commit kernels, beside their openings
    {
        for (uint32_t s = 0; s < G; s++) {
            zip_ctx *ctx = m->shard[s];
            if (hipSetDevice(ctx->device) != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, "hipSetDevice failed"));
            if (!m->roots_all[s] && (rc = pool_alloc(ctx, (size_t)R * 32, (void **)&m->roots_all[s]))) return finish(mfail(m, rc, "roots", ctx));
        }
        bool even = true;
        for (uint32_t s = 0; s < G; s++) even &= m->shard[s]->rows_local == m->shard[0]->rows_local;
        bool done = false;
        if (!m->nccl_comm.empty()) {
            rccl::Api &N = rccl::api();
            int e = (int)N.group_start();
            for (uint32_t s = 0; s < G && e == 0; s++) {
                zip_ctx *ctx = m->shard[s];
                (void)hipSetDevice(ctx->device);
                if (even) {
                    e = (int)N.all_gather(com[s]->roots, m->roots_all[s], (size_t)ctx->rows_local * 32, rccl::kUint8,
                                          static_cast<rccl::comm_t>(m->nccl_comm[s]), ctx->s_commit);
                } else {  // uneven blocks of rows (3 shards): one broadcast per owner
                    for (uint32_t root = 0; root < G && e == 0; root++) {
                        zip_ctx *rc_ = m->shard[root];
                        e = (int)N.broadcast(com[root]->roots, m->roots_all[s] + (size_t)rc_->p.row_begin * 32, (size_t)rc_->rows_local * 32,
                                             rccl::kUint8, (int)root, static_cast<rccl::comm_t>(m->nccl_comm[s]), ctx->s_commit);
                    }
                }
            }
            const int e2 = (int)N.group_end();
            if (e == 0 && e2 == 0) {
                done = true;
                m->roots_path = "rccl";
            } else {
                m->last_error = std::string("RCCL roots gather failed (falling back to copies): ") + (N.err_str ? N.err_str((rccl::result_t)(e ? e : e2)) : "?");
            }
        }
        if (!done) {
            // device copies: every destination pulls every owner's slice once that owner's commit has finished
            for (uint32_t s = 0; s < G; s++) {
                zip_ctx *ctx = m->shard[s];
                if (hipSetDevice(ctx->device) != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, "hipSetDevice failed"));
                for (uint32_t o = 0; o < G; o++) {
                    zip_ctx *oc = m->shard[o];
                    hipError_t e = com[o]->done ? hipStreamWaitEvent(ctx->s_commit, com[o]->done, 0) : hipSuccess;
                    if (e == hipSuccess)
                        e = hipMemcpyPeerAsync(m->roots_all[s] + (size_t)oc->p.row_begin * 32, ctx->device, com[o]->roots, oc->device,
                                               (size_t)oc->rows_local * 32, ctx->s_commit);
                    if (e != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, hipGetErrorString(e)));
                }
            }
            m->roots_path = "copies";
        }
    }
    // ---- 2. lead shard: pull the partial rows together and add them up (exactly)
    if (hipSetDevice(lead->device) != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, "hipSetDevice failed"));
    if (!m->uparts_all && (rc = pool_alloc(lead, (size_t)64 * C * 8 * 8, (void **)&m->uparts_all))) return finish(mfail(m, rc, "partials", lead));
    if (!m->fparts_all && (rc = pool_alloc(lead, (size_t)64 * C * 8 * 8, (void **)&m->fparts_all))) return finish(mfail(m, rc, "partials", lead));
    if (m->ends_cap < u_bytes + row_bytes + 64) {
        pool_release(lead, m->ends);
        m->ends = nullptr;
        if ((rc = pool_alloc(lead, u_bytes + row_bytes + 64, (void **)&m->ends))) return finish(mfail(m, rc, "ends", lead));
        m->ends_cap = u_bytes + row_bytes + 64;
    }
    for (uint32_t s = 0; s < G; s++) {
        zip_ctx *ctx = m->shard[s];
        hipError_t e = hipStreamWaitEvent(lead->stream, m->combined[s], 0);
        if (e == hipSuccess && !single)
            e = hipMemcpyPeerAsync(m->uparts_all + (size_t)s * C * ml, lead->device, m->upart[s], ctx->device, u_bytes, lead->stream);
        if (e == hipSuccess)
            e = hipMemcpyPeerAsync(m->fparts_all + (size_t)s * C * fl, lead->device, m->fpart[s], ctx->device, row_bytes, lead->stream);
        if (e != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, hipGetErrorString(e)));
    }
    {
        const dim3 grid((C + 255) / 256), block(256);
        uint64_t *up = single ? nullptr : reinterpret_cast<uint64_t *>(m->ends);
        const uint64_t *ua = single ? nullptr : m->uparts_all;
        uint8_t *row_be = m->ends + u_bytes;
        LaunchTimer t(lead, "sum_partials_kernel");
        with_fl(fl, [&](auto FL) {
            constexpr int N = decltype(FL)::value;
            hipLaunchKernelGGL(sum_partials_kernel<N>, grid, block, 0, lead->stream, ua, m->fparts_all, G, C, ml, up, (uint64_t *)nullptr, to_dev<N>(hf), row_be);
        });
        if (hipGetLastError() != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, "sum_partials launch failed"));
    }
    m->last_cols = n_cols;
    m->last_fl = fl;
    // ---- 3. results to the host: every shard sends its own rows over its own link
    for (uint32_t s = 0; s < G; s++) {
        zip_ctx *ctx = m->shard[s];
        if (hipSetDevice(ctx->device) != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, "hipSetDevice failed"));
        // (a wait of the pipelined gather that gave up is redone here; synchronises the shard's stream)
        if ((rc = recover_gather_timeout(com[s], cols_dv[s], n_cols, m->slice[s]))) return finish(mfail(m, rc, "openings", ctx));
        const uint32_t rows = ctx->rows_local, r0 = ctx->p.row_begin;
        hipError_t e = hipSuccess;
        if (roots_out) {
            if ((rc = wait_ready(com[s], ctx->stream))) return finish(mfail(m, rc, "roots", ctx));
            e = hipMemcpyAsync(roots_out + (size_t)r0 * 32, com[s]->roots, (size_t)rows * 32, hipMemcpyDeviceToHost, ctx->stream);
        }
        if (e == hipSuccess && proof_out && n_cols) {
            const size_t sp = (size_t)rows * (32 + rec);  // pitch of the shard's slice: one column
            uint8_t *dst = proof_out + u_bytes;
            e = hipMemcpy2DAsync(dst + (size_t)r0 * 32, per_col, m->slice[s], sp, (size_t)rows * 32, n_cols, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess)
                e = hipMemcpy2DAsync(dst + (size_t)R * 32 + (size_t)r0 * rec, per_col, m->slice[s] + (size_t)rows * 32, sp,
                                     (size_t)rows * rec, n_cols, hipMemcpyDeviceToHost, ctx->stream);
        }
        if (e != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, hipGetErrorString(e)));
    }
    if (proof_out) {
        if (hipSetDevice(lead->device) != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, "hipSetDevice failed"));
        hipError_t e = hipSuccess;
        if (u_bytes) e = hipMemcpyAsync(proof_out, m->ends, u_bytes, hipMemcpyDeviceToHost, lead->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(proof_out + u_bytes + (size_t)n_cols * per_col, m->ends + u_bytes, row_bytes, hipMemcpyDeviceToHost, lead->stream);
        if (e != hipSuccess) return finish(mfail(m, ZIP_ERR_HIP, hipGetErrorString(e)));
    }
    rc = finish(ZIP_OK);
    for (uint32_t s = 0; s < G && !rc; s++)
        if ((rc = check_timeout(m->shard[s]))) mfail(m, rc, "pipeline", m->shard[s]);
    return rc;
}

int32_t zip_verify(zip_ctx *ctx, const uint8_t *roots, const uint8_t *proof, zip_mem_kind proof_kind, size_t proof_len,
                   const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont,
                   const uint64_t *q1_mont, const uint64_t *eval_mont, const zip_field *field,
                   zip_verify_report *report) {
    if (!ctx || !roots || !proof || !report || !eval_mont || (n_cols && !cols)) return ZIP_ERR_NULL;
    memset(report, 0, sizeof *report);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (two_limb(ctx))
        return tl_verify(ctx, roots, proof, proof_kind, proof_len, coeffs, cols, n_cols, q0_mont, q1_mont, eval_mont, field, report);
    if (ctx->rows_local != ctx->p.num_rows)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_verify needs an unsharded ctx");
    HostField hf;
    int32_t rc;
    if ((rc = check_verify_args(ctx, coeffs, cols, n_cols, q0_mont, q1_mont, field, &hf))) return rc;
    const size_t need = zip_proof_len(ctx, n_cols, hf.fl);
    if (proof_len < need) {  // the reference runs out of stream: read_* fails (pcs_transcript.rs:125-160)
        report->verdict = ZIP_VERIFY_MALFORMED;
        return ZIP_OK;
    }
    Scratch pbuf(ctx), small(ctx);
    VerifyIn in{};
    if ((rc = stage_verify_inputs(ctx, 1, need, proof, proof_kind, roots, coeffs, cols, n_cols, q0_mont, q1_mont, nullptr, hf.fl,
                                  pbuf, small, &in, proximity_tests(ctx))))
        return rc;
    std::vector<uint32_t> flags, bad, malformed;
    VerifyHead cnt{};
    if ((rc = with_fl(hf.fl, [&](auto FL) { return run_verify_fl<decltype(FL)::value>(ctx, in, hf, flags, bad, malformed, &cnt); })))
        return rc;
    VerifyFacts x{};
    x.overflow = cnt.overflow != 0;
    x.first = x.first_q0 = kNoOpening;
    for (uint32_t i = 0; i < n_cols; i++) {
        report->bad_merkle_paths += bad[i];
        report->malformed_paths += malformed[i];
        const uint32_t why = opening_fails(flags[i], malformed[i], bad[i]);
        if (why && x.first == kNoOpening) {
            x.first = i;
            x.first_why = why;
        }
        if ((flags[i] & 2u) && x.first_q0 == kNoOpening) x.first_q0 = i;
    }
    // <row, q1> is a Montgomery product per element and therefore well defined for elements >= q too; it is 0 for a
    // one-column matrix
    const uint64_t zero[4] = {0, 0, 0, 0};
    x.eval_differs = memcmp(ctx->p.row_len > 1 ? cnt.dot : zero, eval_mont, 8 * hf.fl) != 0;
    x.noncanonical = cnt.noncanonical != 0;
    verify_verdict(x, *report);
    return ZIP_OK;
}

// The batched verifier: MultilinearZip::batch_verify_z (verify_z.rs:40-58) once the caller has walked the shared
// transcript (see zip_hip.h).  Stream i starts at byte i * zip_proof_len of `proofs`; a stream that does not lie wholly
// inside proofs_len is malformed, as it is for zip_verify, and never reaches the device.
int32_t zip_batch_verify(zip_ctx *ctx, uint32_t n_polys, const uint8_t *roots, const uint8_t *proofs, zip_mem_kind proofs_kind,
                         size_t proofs_len, const int64_t *coeffs, const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont,
                         const uint64_t *q1_mont, const uint64_t *evals_mont, const zip_field *field, zip_verify_report *reports) {
    if (!ctx || !roots || !proofs || !reports || !evals_mont || (n_cols && !cols)) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (int32_t r = refuse_two_limb(ctx, "zip_batch_verify")) return r;
    const uint32_t R = ctx->p.num_rows, cw = ctx->p.codeword_len;
    if (n_polys == 0 || n_polys > 65535)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "a batch holds 1 .. 65535 polynomials (got %u)", n_polys);
    if (ctx->rows_local != R) return fail(ctx, ZIP_ERR_INVALID_PARAM, "batches need an unsharded ctx");
    if (int32_t r = refuse_extra_tests(ctx, "zip_batch_verify")) return r;
    if (cw > 16384)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "batches serve codewords up to 16384 (got %u): larger proofs are not launch-bound, "
                    "use zip_verify", cw);
    if ((uint64_t)n_polys * n_cols > 0xFFFFFFFFull)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "%u x %u openings exceed 2^32", n_polys, n_cols);
    HostField hf;
    int32_t rc;
    if ((rc = check_verify_args(ctx, coeffs, cols, n_polys * n_cols, q0_mont, q1_mont, field, &hf))) return rc;
    memset(reports, 0, (size_t)n_polys * sizeof *reports);
    // the reference runs out of stream in the first polynomial that is not all there (pcs_transcript.rs:125-160)
    const size_t len = zip_proof_len(ctx, n_cols, hf.fl);
    const uint32_t k = (uint32_t)std::min<size_t>(n_polys, proofs_len / len);
    for (uint32_t i = k; i < n_polys; i++) reports[i].verdict = ZIP_VERIFY_MALFORMED;
    if (k == 0) return ZIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Scratch pbuf(ctx), small(ctx);
    VerifyIn in{};
    if ((rc = stage_verify_inputs(ctx, k, len, proofs, proofs_kind, roots, coeffs, cols, n_cols, q0_mont, q1_mont, evals_mont, hf.fl,
                                  pbuf, small, &in)))
        return rc;
    g_batch_verify_calls++;
    return with_fl(hf.fl, [&](auto FL) { return run_batch_verify_fl<decltype(FL)::value>(ctx, in, hf, reports); });
}

uint64_t zip_batch_verify_calls(void) { return g_batch_verify_calls.load(); }

// zip_batch_verify for the proofs of a Zinc batch: member i has its own code (slice i of perms1 / perms2), its own field
// and its own stream buffer.  The members share no transcript, so a short stream is that member's matter alone.
int32_t zip_batch_verify_codes(zip_ctx *ctx, uint32_t n_polys, const uint32_t *perms1, const uint32_t *perms2, const uint8_t *roots,
                               const uint8_t *const *proofs, const size_t *proof_lens, zip_mem_kind proofs_kind, const int64_t *coeffs,
                               const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const uint64_t *q1_mont,
                               const uint64_t *evals_mont, const zip_field *const *fields, zip_verify_report *reports) {
    if (!ctx || !roots || !proofs || !proof_lens || !reports || !evals_mont || (n_cols && !cols)) return ZIP_ERR_NULL;
    if (!perms1 || !perms2) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (int32_t r = refuse_two_limb(ctx, "zip_batch_verify_codes")) return r;
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len, cw = ctx->p.codeword_len;
    if (n_polys == 0 || n_polys > 65535)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "a batch holds 1 .. 65535 polynomials (got %u)", n_polys);
    if (ctx->rows_local != R) return fail(ctx, ZIP_ERR_INVALID_PARAM, "batches need an unsharded ctx");
    if (int32_t r = refuse_extra_tests(ctx, "zip_batch_verify_codes")) return r;
    if (cw > 16384)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "batches serve codewords up to 16384 (got %u): larger proofs are not launch-bound, "
                    "use zip_verify", cw);
    if ((uint64_t)n_polys * n_cols > 0xFFFFFFFFull)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "%u x %u openings exceed 2^32", n_polys, n_cols);
    // where zip_batch_verify looks at its field: the members' fields, by zip_batch_open_fields's rules
    std::vector<HostField> hfs;
    int32_t rc;
    if ((rc = batch_member_fields(ctx, fields, n_polys, &hfs))) return rc;
    const uint32_t fl = hfs[0].fl;
    if (R > 1 && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if (C > 1 && !q1_mont) return fail(ctx, ZIP_ERR_NULL, "q1_mont is NULL");
    if ((rc = check_cols(ctx, cols, n_polys * n_cols))) return rc;
    const size_t len = zip_proof_len(ctx, n_cols, fl);
    // a member whose stream is all there must have one; a DEVICE stream is read in place with 8-byte loads
    for (uint32_t i = 0; i < n_polys; i++) {
        if (proof_lens[i] < len) continue;
        if (!proofs[i]) return fail(ctx, ZIP_ERR_NULL, "proofs[%u] is NULL", i);
        if (proofs_kind != ZIP_MEM_HOST && (reinterpret_cast<uintptr_t>(proofs[i]) & 7))
            return fail(ctx, ZIP_ERR_INVALID_PARAM, "member %u: a device stream must be 8-byte aligned", i);
    }
    {   // zip_ctx_create's test of a permutation, per member: the encode kernel indexes with these values
        std::vector<uint8_t> seen(cw);
        for (uint32_t i = 0; i < n_polys; i++)
            for (int k = 0; k < 2; k++) {
                const uint32_t *perm = (k ? perms2 : perms1) + (size_t)i * cw;
                std::fill(seen.begin(), seen.end(), 0);
                for (uint32_t j = 0; j < cw; j++) {
                    if (perm[j] >= cw || seen[perm[j]])
                        return fail(ctx, ZIP_ERR_INVALID_PARAM, "member %u: perm%d is not a permutation of [0, %u)", i, k + 1, cw);
                    seen[perm[j]] = 1;
                }
            }
    }
    memset(reports, 0, (size_t)n_polys * sizeof *reports);
    // the members that reach the device; a short stream is malformed as it is for zip_verify (pcs_transcript.rs:125-160)
    std::vector<uint32_t> live;
    live.reserve(n_polys);
    for (uint32_t i = 0; i < n_polys; i++) {
        if (proof_lens[i] < len) reports[i].verdict = ZIP_VERIFY_MALFORMED;
        else live.push_back(i);
    }
    const uint32_t k = (uint32_t)live.size();
    if (k == 0) return ZIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    g_batch_verify_codes_calls++;
    g_batch_verify_codes_members += k;
    // the small inputs of the live members, contiguous: the caller's arrays when every member is live
    const bool all = k == n_polys;
    const bool single = R == 1;
    std::vector<unsigned char> packed[8];
    std::vector<HostField> live_hf;
    auto gather = [&](int slot, const void *src, size_t per_member) -> const void * {
        if (all || !src || !per_member) return src;
        packed[slot].resize((size_t)k * per_member);
        for (uint32_t j = 0; j < k; j++)
            memcpy(packed[slot].data() + (size_t)j * per_member, static_cast<const unsigned char *>(src) + (size_t)live[j] * per_member, per_member);
        return packed[slot].data();
    };
    if (!all)
        for (uint32_t j = 0; j < k; j++) live_hf.push_back(hfs[live[j]]);
    const std::vector<HostField> &mhf = all ? hfs : live_hf;
    Scratch pbuf(ctx), perms(ctx), small(ctx);
    // the codes, once: all perm1 slices of the live members, then all perm2 slices
    const size_t perm_words = (size_t)k * cw;
    if ((rc = perms.get(2 * perm_words * 4))) return rc;
    uint32_t *perms_d = perms.as<uint32_t>();
    if ((rc = copy_h2d_bounced(ctx, perms_d, gather(6, perms1, (size_t)cw * 4), perm_words * 4, ctx->stream))) return rc;
    if ((rc = copy_h2d_bounced(ctx, perms_d + perm_words, gather(7, perms2, (size_t)cw * 4), perm_words * 4, ctx->stream))) return rc;
    std::vector<const uint8_t *> streams(k);
    if (proofs_kind == ZIP_MEM_HOST) {  // stream j into its slot of one pooled block
        if ((rc = pbuf.get((size_t)k * len))) return rc;
        for (uint32_t j = 0; j < k; j++) {
            streams[j] = pbuf.as<uint8_t>() + (size_t)j * len;
            if ((rc = copy_h2d_bounced(ctx, pbuf.as<uint8_t>() + (size_t)j * len, proofs[live[j]], len, ctx->stream))) return rc;
        }
    } else {
        for (uint32_t j = 0; j < k; j++) streams[j] = proofs[live[j]];
    }
    std::vector<unsigned char> inst_h;
    with_fl(fl, [&](auto FL) { batch_fill_verify_members<decltype(FL)::value>(mhf, streams, perms_d, perms_d + perm_words, cw, &inst_h); });
    SmallInputs si;
    si.src[0] = gather(0, coeffs, (size_t)R * 8);          si.bytes[0] = single ? 0 : (size_t)k * R * 8;
    si.src[1] = gather(1, q0_mont, (size_t)R * fl * 8);    si.bytes[1] = single ? 0 : (size_t)k * R * fl * 8;
    si.src[2] = gather(2, cols, (size_t)n_cols * 4);       si.bytes[2] = (size_t)k * n_cols * 4;
    si.src[3] = gather(3, q1_mont, (size_t)C * fl * 8);    si.bytes[3] = C > 1 ? (size_t)k * C * fl * 8 : 0;
    si.src[4] = gather(4, roots, (size_t)R * 32);          si.bytes[4] = (size_t)k * R * 32;
    si.src[5] = gather(5, evals_mont, (size_t)fl * 8);     si.bytes[5] = (size_t)k * fl * 8;
    si.src[6] = inst_h.data();                             si.bytes[6] = inst_h.size();
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    VerifyIn in{};
    in.coeffs_d = reinterpret_cast<const int64_t *>(sb + si.off[0]);
    in.q0_d = reinterpret_cast<const uint64_t *>(sb + si.off[1]);
    in.cols_d = reinterpret_cast<const uint32_t *>(sb + si.off[2]);
    in.q1_d = reinterpret_cast<const uint64_t *>(sb + si.off[3]);
    in.roots_d = sb + si.off[4];
    in.evals_d = reinterpret_cast<const uint64_t *>(sb + si.off[5]);
    in.n_cols = n_cols;
    in.n_polys = k;
    std::vector<zip_verify_report> live_reports(all ? 0 : k);
    zip_verify_report *dst = all ? reports : live_reports.data();
    if ((rc = with_fl(fl, [&](auto FL) { return run_batch_verify_codes_fl<decltype(FL)::value>(ctx, in, sb + si.off[6], dst); })))
        return rc;
    if (!all)
        for (uint32_t j = 0; j < k; j++) reports[live[j]] = live_reports[j];
    return ZIP_OK;
}

void zip_batch_verify_codes_counts(uint64_t *calls, uint64_t *members) {
    if (calls) *calls = g_batch_verify_codes_calls.load();
    if (members) *members = g_batch_verify_codes_members.load();
}

int32_t zip_commitment_mle_eval(zip_commitment *c, const uint64_t *q0_mont, const uint64_t *q1_mont,
                                const zip_field *field, uint64_t *value_out) {
    if (!c) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    if (!c->evals)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "the commitment holds no witness (it was committed from device memory or uploaded)");
    // c->evals went up on s_commit, and zip_commit waited for that stream before it returned
    return zip_mle_eval(ctx, c->evals, ZIP_MEM_DEVICE, q0_mont, q1_mont, field, value_out);
}

int32_t zip_mle_eval(zip_ctx *ctx, const int64_t *evals, zip_mem_kind evals_kind, const uint64_t *q0_mont,
                     const uint64_t *q1_mont, const zip_field *field, uint64_t *value_out) {
    if (!ctx || !value_out) return ZIP_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (two_limb(ctx)) return tl_open_eval(ctx, evals, evals_kind, q0_mont, q1_mont, field, nullptr, ZIP_MEM_HOST, value_out);
    if (ctx->rows_local != ctx->p.num_rows)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_mle_eval needs an unsharded ctx");
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    const uint32_t R = ctx->p.num_rows, C = ctx->p.row_len;
    const bool single = R == 1;
    if (!single && !q0_mont) return fail(ctx, ZIP_ERR_NULL, "q0_mont is NULL");
    if (C > 1 && !q1_mont) return fail(ctx, ZIP_ERR_NULL, "q1_mont is NULL");
    Scratch ev(ctx), row(ctx), small(ctx), res(ctx);
    const int64_t *evals_d;
    if ((rc = stage_evals(ctx, evals, evals_kind, (size_t)R * C, ev, &evals_d))) return rc;
    if ((rc = row.get((size_t)C * hf.fl * 8))) return rc;
    if ((rc = res.get(64))) return rc;
    SmallInputs si;
    si.src[1] = single ? hf.r : q0_mont;
    si.bytes[1] = (size_t)R * hf.fl * 8;
    si.src[3] = C > 1 ? (const void *)q1_mont : (const void *)hf.r;  // a one-column matrix evaluates to its entry
    si.bytes[3] = (size_t)C * hf.fl * 8;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    CombineOut o{};
    o.row_limbs = row.as<uint64_t>();
    if ((rc = run_combine(ctx, evals_d, nullptr, reinterpret_cast<const uint64_t *>(sb + si.off[1]), &hf, false, true, o)))
        return rc;
    {
        LaunchTimer t(ctx, "field_dot_kernel");
        const uint64_t *q1d = reinterpret_cast<const uint64_t *>(sb + si.off[3]);
        with_fl(hf.fl, [&](auto FL) {
            constexpr int N = decltype(FL)::value;
            hipLaunchKernelGGL(field_dot_kernel<N>, dim3(1), dim3(1024), 0, ctx->stream, o.row_limbs, q1d, C, res.as<uint64_t>(), to_dev<N>(hf));
        });
        HIP_TRY(ctx, hipGetLastError());
    }
    return deliver(ctx, value_out, ZIP_MEM_HOST, res.ptr, (size_t)hf.fl * 8);
}

int32_t zip_field_map_int256(zip_ctx *ctx, const uint64_t *values, uint32_t n, const zip_field *field, uint64_t *out) {
    if (!ctx || !values || !out) return ZIP_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    Scratch in(ctx), res(ctx);
    if ((rc = in.get((size_t)n * 32 + 16))) return rc;
    if ((rc = res.get((size_t)n * hf.fl * 8 + 16))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(in.ptr, values, (size_t)n * 32, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((n + 255) / 256), block(256);
    with_fl(hf.fl, [&](auto FL) {
        constexpr int N = decltype(FL)::value;
        const VerifyField<N> vf = verify_field<N>(hf);
        hipLaunchKernelGGL(field_map_int256_kernel<N>, grid, block, 0, ctx->stream, in.as<uint64_t>(), n, res.as<uint64_t>(), vf.fd, vf.fq, vf.quirk);
    });
    HIP_TRY(ctx, hipGetLastError());
    return deliver(ctx, out, ZIP_MEM_HOST, res.ptr, (size_t)n * hf.fl * 8);
}

// Diagnostic beside zip_field_map_int256: phi of Int<2> (the two-limb witness map) and Int<8> (the verifier's map of a
// two-limb ctx's column entries) values, on any ctx
int32_t zip_field_map_int(zip_ctx *ctx, const uint64_t *values, uint32_t n, uint32_t value_limbs, const zip_field *field, uint64_t *out) {
    if (!ctx || !values || !out) return ZIP_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (value_limbs != 2 && value_limbs != 8)
        return fail(ctx, ZIP_ERR_UNSUPPORTED, "zip_field_map_int maps Int<2> and Int<8> values (got %u limbs)", value_limbs);
    return tl_field_map_int(ctx, values, n, value_limbs, field, out);
}

int32_t zip_open_stream(zip_commitment *c, const int64_t *evals, zip_mem_kind evals_kind, const int64_t *coeffs,
                        const uint32_t *cols, uint32_t n_cols, const uint64_t *q0_mont, const zip_field *field,
                        zip_proof_sink sink, void *user, size_t chunk_bytes) {
    if (!c || !sink || (n_cols && !cols)) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (int32_t r = refuse_two_limb(ctx, "zip_open_stream")) return r;
    if (ctx->rows_local != ctx->p.num_rows)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_open_stream needs an unsharded ctx");
    if (!c->layers) return fail(ctx, ZIP_ERR_INVALID_PARAM, "commitment has no Merkle trees (commit_no_merkle)");
    HostField hf;
    int32_t rc;
    if ((rc = make_field(ctx, field, &hf))) return rc;
    const bool single = ctx->p.num_rows == 1;
    if (!single && (!coeffs || !q0_mont)) return fail(ctx, ZIP_ERR_NULL, "coeffs / q0_mont is NULL");
    if ((rc = check_cols(ctx, cols, n_cols))) return rc;
    Scratch ev(ctx), ends(ctx), small(ctx), dev0(ctx), dev1(ctx);
    const int64_t *evals_d = c->evals;
    if (evals) {
        if ((rc = stage_evals(ctx, evals, evals_kind, (size_t)ctx->rows_local * ctx->p.row_len, ev, &evals_d))) return rc;
    } else if (!evals_d) {
        return fail(ctx, ZIP_ERR_NULL, "evals is NULL and the commitment retains no witness");
    }
    if ((rc = ensure_columns(c, cols, n_cols, evals_d))) return rc;
    note_columns(ctx, cols, n_cols);
    const uint32_t T = proximity_tests(ctx);
    const size_t u_bytes = uprime_bytes(ctx);  // u'_0 .. u'_{T-1}: the first piece
    const size_t row_bytes = (size_t)ctx->p.row_len * hf.fl * 8;
    const size_t colb = column_bytes(ctx);
    // columns per group: as many as fit the hint (default 64 MiB), at least one
    if (chunk_bytes == 0) chunk_bytes = (size_t)64 << 20;
    size_t group = colb ? chunk_bytes / colb : n_cols;
    if (group < 1) group = 1;
    if (group > n_cols) group = n_cols ? n_cols : 1;
    const size_t buf_bytes = std::max(group * colb, std::max(u_bytes, row_bytes));
    if ((rc = ensure_bounce(ctx, buf_bytes))) return rc;
    if ((rc = ends.get(u_bytes + row_bytes + 16))) return rc;
    if ((rc = dev0.get(group * colb + 16))) return rc;
    if ((rc = dev1.get(group * colb + 16))) return rc;
    uint8_t *dev[2] = {dev0.as<uint8_t>(), dev1.as<uint8_t>()};
    SmallInputs si;
    if (!single) {
        si.src[0] = coeffs;
        si.bytes[0] = (size_t)T * ctx->rows_local * 8;
    }
    si.src[1] = single ? hf.r : q0_mont;
    si.bytes[1] = (size_t)ctx->rows_local * hf.fl * 8;
    si.src[2] = cols;
    si.bytes[2] = (size_t)n_cols * 4;
    unsigned char *sb;
    if ((rc = stage_small(ctx, si, small, &sb))) return rc;
    const uint32_t *cols_d = reinterpret_cast<const uint32_t *>(sb + si.off[2]);
    // the two row combinations (they do not need the commitment) -> u' and the evaluation row
    CombineOut o{};
    o.uprime = single ? nullptr : ends.as<uint64_t>();
    o.row_be = ends.as<uint8_t>() + u_bytes;
    if ((rc = run_combine(ctx, evals_d, reinterpret_cast<const int64_t *>(sb + si.off[0]),
                          reinterpret_cast<const uint64_t *>(sb + si.off[1]), &hf, !single, true, o)))
        return rc;
    if (T > 1 && (rc = run_combine_extra(ctx, evals_d, reinterpret_cast<const int64_t *>(sb + si.off[0]) + ctx->rows_local, T - 1,
                                         o.uprime + (size_t)ctx->p.row_len * ctx->p.m_limbs)))
        return rc;
    hipStream_t s_copy = ctx->s_upper;  // D2H copies run beside the next group's gather
    hipEvent_t gathered[2] = {take_dep_event(ctx), take_dep_event(ctx)};
    hipEvent_t copied[2] = {take_dep_event(ctx), take_dep_event(ctx)};
    for (int i = 0; i < 2; i++) { c->aux.push_back(gathered[i]); c->aux.push_back(copied[i]); }
    // piece 1: u' (open_z.rs:110-112)
    if (u_bytes) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->bounce[0], ends.ptr, u_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, stream_wait(ctx->stream));
        if (sink(user, ctx->bounce[0], u_bytes)) return fail(ctx, ZIP_ERR_INVALID_PARAM, "the proof sink refused the stream");
    }
    if ((rc = wait_ready(c, ctx->stream))) return rc;
    // pieces 2..: groups of opened columns, double buffered: gather g+1 | copy g | sink g-1
    const size_t n_groups = n_cols ? (n_cols + group - 1) / group : 0;
    auto launch = [&](size_t g) -> int32_t {
        const int b = (int)(g & 1);
        const uint32_t first = (uint32_t)(g * group), cnt = (uint32_t)std::min(group, (size_t)n_cols - first);
        if (g >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, copied[b], 0));  // dev[b] has left the device
        int32_t r = run_open_columns(c, cols_d + first, cnt, dev[b], 0, ctx->rows_local, first);
        if (r) return r;
        HIP_TRY(ctx, hipEventRecord(gathered[b], ctx->stream));
        return ZIP_OK;
    };
    auto copy_out = [&](size_t g) -> int32_t {
        const int b = (int)(g & 1);
        const uint32_t first = (uint32_t)(g * group), cnt = (uint32_t)std::min(group, (size_t)n_cols - first);
        HIP_TRY(ctx, hipStreamWaitEvent(s_copy, gathered[b], 0));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->bounce[b], dev[b], (size_t)cnt * colb, hipMemcpyDeviceToHost, s_copy));
        HIP_TRY(ctx, hipEventRecord(copied[b], s_copy));
        return ZIP_OK;
    };
    int32_t status = ZIP_OK;
    if (n_groups) status = launch(0);
    for (size_t g = 0; g < n_groups && status == ZIP_OK; g++) {
        // bounce[g & 1] is free: the sink of group g-2 returned before this iteration began
        if ((status = copy_out(g))) break;
        if (g + 1 < n_groups && (status = launch(g + 1))) break;
        if (event_wait(copied[g & 1]) != hipSuccess) { status = fail(ctx, ZIP_ERR_HIP, "proof copy failed"); break; }
        const uint32_t first = (uint32_t)(g * group), cnt = (uint32_t)std::min(group, (size_t)n_cols - first);
        if (sink(user, ctx->bounce[g & 1], (size_t)cnt * colb))
            status = fail(ctx, ZIP_ERR_INVALID_PARAM, "the proof sink refused the stream");
    }
    // drain whatever is still in flight before the scratch buffers return to the pool
    (void)stream_wait(s_copy);
    HIP_TRY(ctx, stream_wait(ctx->stream));
    if (status) return status;
    // last piece: the evaluation row (open_z.rs:89-90)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->bounce[0], ends.as<uint8_t>() + u_bytes, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    if (sink(user, ctx->bounce[0], row_bytes)) return fail(ctx, ZIP_ERR_INVALID_PARAM, "the proof sink refused the stream");
    return check_timeout(ctx);
}

namespace {
// The private plumbing context of a sumcheck or CCS handle, or of one call: `device` made current, its CU count, a
// non-blocking stream; recycle: the blocks come from the device's recycle bin and go back there.  An error leaves no
// context behind.
int32_t private_ctx_create(int32_t device, bool recycle, zip_ctx **out) {
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return ZIP_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return ZIP_ERR_NO_DEVICE;
    zip_ctx *ctx = new (std::nothrow) zip_ctx();
    if (!ctx) return ZIP_ERR_ALLOC;
    ctx->device = device;
    ctx->recycle = recycle;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        ctx->num_cus = (uint32_t)cus;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;  // (nothing but the object exists yet)
        return ZIP_ERR_HIP;
    }
    *out = ctx;
    return ZIP_OK;
}
}  // namespace

static int32_t sumcheck_create(int32_t device, const uint64_t *const *mles, zip_mem_kind kind, uint32_t n_mles, uint32_t num_vars,
                               uint32_t degree, const zip_sumcheck_comb *comb, bool products, const zip_field *field,
                               zip_sumcheck **out);

int32_t zip_sumcheck_init(int32_t device, const uint64_t *const *mles, zip_mem_kind kind, uint32_t n_mles,
                          uint32_t num_vars, uint32_t degree, const zip_sumcheck_comb *comb, const zip_field *field,
                          zip_sumcheck **out) {
    if (!mles || !out || !field) return ZIP_ERR_NULL;
    *out = nullptr;
    if (comb && (comb->n_terms < 1 || comb->n_terms > 8)) return ZIP_ERR_INVALID_PARAM;
    if (n_mles < 1 || n_mles > (uint32_t)kSumcheckMaxMles || degree < 1 || degree > (uint32_t)kSumcheckMaxDegree ||
        num_vars < 1 || num_vars > 30)
        return ZIP_ERR_INVALID_PARAM;  // nvars == 0: "Attempt to prove a constant." (prover.rs:47-49)
    if (comb)  // a term that refers to an MLE that does not exist
        for (uint32_t t = 0; t < comb->n_terms; t++)
            if (comb->term_mask[t] >> n_mles) return ZIP_ERR_INVALID_PARAM;
    return sumcheck_create(device, mles, kind, n_mles, num_vars, degree, comb, false, field, out);
}

int32_t zip_sumcheck_init_products(int32_t device, const uint64_t *const *mles, zip_mem_kind kind, uint32_t n_mles,
                                   uint32_t num_vars, uint32_t degree, const zip_sumcheck_comb *products,
                                   const zip_field *field, zip_sumcheck **out) {
    if (!mles || !out || !field) return ZIP_ERR_NULL;
    *out = nullptr;
    if (!products) return ZIP_ERR_NULL;
    if (products->n_terms < 1 || products->n_terms > 8) return ZIP_ERR_INVALID_PARAM;
    if (n_mles < 1 || n_mles > (uint32_t)kSumcheckProductsMaxMles || degree < 1 || degree > (uint32_t)kSumcheckMaxDegree ||
        num_vars < 1 || num_vars > 30)
        return ZIP_ERR_INVALID_PARAM;
    for (uint32_t t = 0; t < products->n_terms; t++) {  // 1..4 multiplicands, all of them among the tables
        const uint32_t m = products->term_mask[t];
        const int bits = __builtin_popcount(m);
        if (bits < 1 || bits > kSumcheckProductsMaxFactors || ((uint64_t)m >> n_mles)) return ZIP_ERR_INVALID_PARAM;
    }
    return sumcheck_create(device, mles, kind, n_mles, num_vars, degree, products, true, field, out);
}

// what zip_sumcheck_init and zip_sumcheck_init_products share: the arguments have been checked
static int32_t sumcheck_create(int32_t device, const uint64_t *const *mles, zip_mem_kind kind, uint32_t n_mles, uint32_t num_vars,
                               uint32_t degree, const zip_sumcheck_comb *comb, bool products, const zip_field *field,
                               zip_sumcheck **out) {
    zip_ctx *ctx = nullptr;
    int32_t rc = private_ctx_create(device, true, &ctx);
    if (rc) return rc;
    zip_sumcheck *s = new (std::nothrow) zip_sumcheck();
    if (!s) { zip_ctx_destroy(ctx); return ZIP_ERR_ALLOC; }
    s->ctx = ctx;
    do {
        HostField &hf = s->field;
        if ((rc = make_field(ctx, field, &hf))) break;
        s->n_mles = n_mles;
        s->num_vars = num_vars;
        s->degree = degree;
        s->fl = hf.fl;
        if (comb) {
            s->n_terms = comb->n_terms;
            for (uint32_t t = 0; t < comb->n_terms; t++) {
                s->term_mask[t] = comb->term_mask[t];
                memcpy(s->coeff[t], comb->coeff[t], sizeof s->coeff[t]);
            }
        }
        uint32_t used = n_mles >= 32 ? ~0u : (1u << n_mles) - 1u;  // the tables that are read at all
        if (products) {
            // factor lists, and who writes the folded table of an MLE that several products share: the lowest-numbered one
            s->products = true;
            used = 0;
            for (uint32_t t = 0; t < comb->n_terms; t++) {
                uint32_t nf = 0, first = 0;
                for (uint32_t k = 0; k < n_mles; k++) {
                    if (!((comb->term_mask[t] >> k) & 1u)) continue;
                    if (nf == 0) first = k;
                    s->factors[t] |= k << (8 * nf);
                    if (!((used >> k) & 1u)) s->own[t] |= 1u << nf;
                    used |= 1u << k;
                    nf++;
                }
                s->n_factors[t] = nf;
                for (uint32_t j = nf; j < (uint32_t)kSumcheckProductsMaxFactors; j++) s->factors[t] |= first << (8 * j);
            }
        }
        const size_t n = (size_t)1 << num_vars, elem = (size_t)hf.fl * 8;
        for (uint32_t k = 0; k < n_mles && rc == ZIP_OK; k++) {
            if (!mles[k]) { rc = ZIP_ERR_NULL; break; }
            if (!((used >> k) & 1u)) continue;  // in no product: neither copied, read nor folded
            if (kind == ZIP_MEM_HOST) {
                void *d = nullptr;
                if ((rc = pool_alloc(ctx, n * elem, &d))) break;
                s->input[k] = static_cast<uint64_t *>(d);
                rc = copy_h2d_bounced(ctx, d, mles[k], n * elem, ctx->stream);
            } else {
                s->input[k] = mles[k];
            }
            if (rc) break;
            if (num_vars >= 2 && (rc = pool_alloc(ctx, (n / 2) * elem, (void **)&s->buf[0][k]))) break;
            if (num_vars >= 3 && (rc = pool_alloc(ctx, (n / 4) * elem, (void **)&s->buf[1][k]))) break;
        }
        if (rc) break;
        s->owned = kind == ZIP_MEM_HOST;
        s->max_blocks = ctx->num_cus * 8;
        if ((rc = pool_alloc(ctx, (size_t)s->max_blocks * (degree + 1) * elem, (void **)&s->partials))) break;
        if ((rc = pool_alloc(ctx, (size_t)(degree + 1) * elem, (void **)&s->evals_d))) break;
        if ((rc = pool_alloc(ctx, 16, (void **)&s->done_d))) break;
        if ((rc = pool_alloc(ctx, kTailOutBytes, (void **)&s->tail_out_d))) break;
        if (hipMemsetAsync(s->done_d, 0, 16, ctx->stream) != hipSuccess) { rc = ZIP_ERR_HIP; break; }
        if (stream_wait(ctx->stream) != hipSuccess) { rc = ZIP_ERR_HIP; break; }
        bounce_release(ctx);                  // the tables are up: nothing else of this handle goes through them
        s->evals_pinned = slab_take(device);  // null (all slots busy): the message goes through evals_d and a copy
        if (s->evals_pinned) memset(s->evals_pinned, 0, kSlabSlotBytes);
    } while (0);
    if (rc) {
        zip_sumcheck_free(s);
        return rc;
    }
    *out = s;
    return ZIP_OK;
}

int32_t zip_sumcheck_round_begin(zip_sumcheck *s, const uint64_t *r_prev) {
    if (!s) return ZIP_ERR_NULL;
    zip_ctx *ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (s->pending) return fail(ctx, ZIP_ERR_INVALID_PARAM, "the previous round has not been collected (zip_sumcheck_round_end)");
    if (s->round >= s->num_vars) return fail(ctx, ZIP_ERR_INVALID_PARAM, "Prover is not active");  // prover.rs:91-93
    if (s->round == 0 && r_prev) return fail(ctx, ZIP_ERR_INVALID_PARAM, "first round should be prover first.");
    if (s->round > 0 && !r_prev) return fail(ctx, ZIP_ERR_INVALID_PARAM, "verifier message is empty");
    if (int32_t rc = with_fl(s->fl, [&](auto FL) {
            return s->products ? sumcheck_round_products_fl<decltype(FL)::value>(s, r_prev)
                               : sumcheck_round_fl<decltype(FL)::value>(s, r_prev);
        }))
        return rc;
    g_sumcheck_round_launches++;
    s->round++;
    s->pending = true;
    return ZIP_OK;
}

int32_t zip_sumcheck_round_end(zip_sumcheck *s, uint64_t *evaluations_out) {
    if (!s || !evaluations_out) return ZIP_ERR_NULL;
    zip_ctx *ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!s->pending) return fail(ctx, ZIP_ERR_INVALID_PARAM, "no round in flight (zip_sumcheck_round_begin)");
    s->pending = false;
    const size_t msg_bytes = (size_t)(s->degree + 1) * s->fl * 8;
    if (s->evals_pinned) {
        // The kernel writes the message, then the round number, into host-mapped coherent memory: poll that word
        // for a while (a stream synchronise costs ~20 us of wake-up latency, forty times per proof), then fall back.
        volatile uint32_t *flag = reinterpret_cast<volatile uint32_t *>(s->evals_pinned + 192);
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        for (uint32_t spin = 0;; spin++) {
            if (*flag == s->round) { seen = true; break; }
            if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300)) break;
        }
        if (seen) std::atomic_thread_fence(std::memory_order_acquire);
        else HIP_TRY(ctx, stream_wait(ctx->stream));
        memcpy(evaluations_out, s->evals_pinned, msg_bytes);
        return ZIP_OK;
    }
    HIP_TRY(ctx, hipMemcpyAsync(evaluations_out, s->evals_d, msg_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

int32_t zip_sumcheck_round(zip_sumcheck *s, const uint64_t *r_prev, uint64_t *evaluations_out) {
    if (!s || !evaluations_out) return ZIP_ERR_NULL;
    const int32_t rc = zip_sumcheck_round_begin(s, r_prev);
    return rc ? rc : zip_sumcheck_round_end(s, evaluations_out);
}

int32_t zip_sumcheck_prove(zip_sumcheck *s, zip_keccak_state *transcript, uint64_t *msgs_out, uint64_t *randomness_out) {
    if (!s || !transcript || !msgs_out || !randomness_out) return ZIP_ERR_NULL;
    zip_ctx *ctx = s->ctx;
    if (s->proved) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_sumcheck_prove has already run on this handle");
    if (s->pending || s->round > 0)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_sumcheck_prove needs a fresh handle: a round has been played or is in flight");
    if (transcript->buflen >= kKeccakRate)
        return fail(ctx, ZIP_ERR_INVALID_PARAM, "transcript buflen %u is not below the Keccak-256 rate (136)", transcript->buflen);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    s->proved = true;  // whatever happens from here on, the handle does not start over
    const int32_t rc = with_fl(s->fl, [&](auto FL) { return sumcheck_prove_fl<decltype(FL)::value>(s, transcript, msgs_out, randomness_out); });
    if (rc) s->round = s->num_vars;
    return rc;
}

void zip_sumcheck_launch_counts(uint64_t *rounds, uint64_t *tails) {
    if (rounds) *rounds = g_sumcheck_round_launches.load();
    if (tails) *tails = g_sumcheck_tail_launches.load();
}

void zip_sumcheck_grid_counts(uint64_t *multi_pass, uint64_t *uneven_last_pass, uint64_t *reduce_kernel) {
    if (multi_pass) *multi_pass = g_sumcheck_multi_pass.load();
    if (uneven_last_pass) *uneven_last_pass = g_sumcheck_uneven_last_pass.load();
    if (reduce_kernel) *reduce_kernel = g_sumcheck_reduce_launches.load();
}

int32_t zip_sumcheck_prove_batch(int32_t device, const zip_sumcheck_instance *inst, uint32_t n_instances, zip_mem_kind tables_kind,
                                 uint32_t n_mles, uint32_t num_vars, uint32_t degree, uint64_t *msgs_out, uint64_t *randomness_out) {
    // usage errors, before anything reaches the device: every NULL first, then the parameters, then the size limit
    if (!inst || !msgs_out || !randomness_out) return ZIP_ERR_NULL;
    const uint32_t scan = std::min<uint32_t>(n_instances, 65535), scan_k = std::min<uint32_t>(n_mles, kSumcheckMaxMles);
    for (uint32_t i = 0; i < scan; i++) {
        if (!inst[i].mles || !inst[i].field || !inst[i].transcript) return ZIP_ERR_NULL;
        for (uint32_t k = 0; k < scan_k; k++)
            if (!inst[i].mles[k]) return ZIP_ERR_NULL;
    }
    if (n_instances < 1 || n_instances > 65535) return ZIP_ERR_INVALID_PARAM;
    if (n_mles < 1 || n_mles > (uint32_t)kSumcheckMaxMles || degree < 1 || degree > (uint32_t)kSumcheckMaxDegree || num_vars < 1 ||
        num_vars > 30)
        return ZIP_ERR_INVALID_PARAM;  // (zip_sumcheck_init's ranges; what lies above this entry point's own is refused below)
    const uint32_t fl = inst[0].field->limbs;
    if (fl < 2 || fl > 4) return ZIP_ERR_INVALID_PARAM;
    for (uint32_t i = 0; i < n_instances; i++)
        if (inst[i].field->limbs != fl) return ZIP_ERR_INVALID_PARAM;
    for (uint32_t i = 0; i < n_instances; i++) {
        const zip_sumcheck_comb *c = inst[i].comb;
        if (!c) continue;
        if (c->n_terms < 1 || c->n_terms > 8) return ZIP_ERR_INVALID_PARAM;
        for (uint32_t t = 0; t < c->n_terms; t++)
            if (c->term_mask[t] >> n_mles) return ZIP_ERR_INVALID_PARAM;
    }
    for (uint32_t i = 0; i < n_instances; i++)
        if (inst[i].transcript->buflen >= kKeccakRate) return ZIP_ERR_INVALID_PARAM;
    if (num_vars > kBatchSumcheckMaxVars) return ZIP_ERR_UNSUPPORTED;
    // FieldConfig::new per instance (an even modulus or 1: ZIP_ERR_INVALID_PARAM, as from zip_sumcheck_init); neighbours
    // with the same modulus share the work
    std::vector<HostField> fields(n_instances);
    for (uint32_t i = 0; i < n_instances; i++) {
        if (i && !memcmp(inst[i].field->modulus, inst[i - 1].field->modulus, 8 * (size_t)fl)) {
            fields[i] = fields[i - 1];
            continue;
        }
        if (int32_t rc = make_field_uncached(nullptr, inst[i].field, &fields[i])) return rc;
    }
    CurrentDeviceGuard restore;
    zip_ctx *ctx = nullptr;  // the call's plumbing, as a zip_sumcheck handle has one
    int32_t rc = private_ctx_create(device, true, &ctx);
    if (rc) return rc;
    rc = with_fl(fl, [&](auto FL) {
        return sumcheck_prove_batch_fl<decltype(FL)::value>(ctx, inst, n_instances, tables_kind, n_mles, num_vars, degree, fields,
                                                            msgs_out, randomness_out);
    });
    zip_ctx_destroy(ctx);  // waits for the stream; every block goes back to the device's recycle bin
    return rc;
}

void zip_sumcheck_batch_counts(uint64_t *launches, uint64_t *instances, uint64_t *streamed_rounds) {
    if (launches) *launches = g_sumcheck_batch_launches.load();
    if (instances) *instances = g_sumcheck_batch_instances.load();
    if (streamed_rounds) *streamed_rounds = g_sumcheck_batch_streamed.load();
}

int32_t zip_prime_test_base2(int32_t device, const uint64_t *candidates, uint32_t n, uint32_t limbs, uint8_t *verdicts_out) {
    if (!candidates || !verdicts_out) return ZIP_ERR_NULL;
    if (limbs < 2 || limbs > 4 || n == 0) return ZIP_ERR_INVALID_PARAM;
    for (uint32_t i = 0; i < n; i++) {  // the lane function's contract: odd, at least 3
        const uint64_t *c = candidates + (size_t)i * limbs;
        uint64_t hi = 0;
        for (uint32_t k = 1; k < limbs; k++) hi |= c[k];
        if (!(c[0] & 1) || (hi == 0 && c[0] < 3)) return ZIP_ERR_INVALID_PARAM;
    }
    if (device < 0 || device >= kMaxDevices) return ZIP_ERR_NO_DEVICE;
    PrimeDev &pd = g_prime[device];
    std::lock_guard<std::mutex> g(pd.mu);
    CurrentDeviceGuard restore;
    if (int32_t rc = prime_dev_ready(pd, device)) return rc;
    return with_fl(limbs, [&](auto FL) { return prime_test_fl<decltype(FL)::value>(pd, candidates, n, verdicts_out); });
}

int32_t zip_get_prime(int32_t device, zip_keccak_state *transcript, uint32_t limbs, uint64_t *prime_out,
                      uint32_t *candidates_tried_out) {
    if (!transcript || !prime_out) return ZIP_ERR_NULL;
    if (limbs < 2 || limbs > 4 || transcript->buflen >= kKeccakRate) return ZIP_ERR_INVALID_PARAM;
    if (device < 0 || device >= kMaxDevices) return ZIP_ERR_NO_DEVICE;
    PrimeDev &pd = g_prime[device];
    std::lock_guard<std::mutex> g(pd.mu);
    CurrentDeviceGuard restore;
    if (int32_t rc = prime_dev_ready(pd, device)) return rc;
    // (per call: the tests flip it)
    const uint32_t batch = prime_batch_knob(getenv("ZIP_HIP_PRIME_BATCH"), kPrimeDefaultBatch, kPrimeMaxBatch);
    return with_fl(limbs, [&](auto FL) {
        return get_prime_fl<decltype(FL)::value>(pd, transcript, batch, prime_out, candidates_tried_out);
    });
}

void zip_prime_launch_counts(uint64_t *launches, uint64_t *candidates_tested) {
    if (launches) *launches = g_prime_launches.load();
    if (candidates_tested) *candidates_tested = g_prime_candidates.load();
}

int32_t zip_get_prime_batch(int32_t device, zip_keccak_state *transcripts, uint32_t n, uint32_t limbs, uint64_t *primes_out,
                            uint32_t *candidates_tried_out) {
    if (!transcripts || !primes_out) return ZIP_ERR_NULL;
    if (limbs < 2 || limbs > 4) return ZIP_ERR_INVALID_PARAM;
    if (n == 0 || n > kPrimeBatchMaxMembers) return ZIP_ERR_INVALID_PARAM;
    for (uint32_t i = 0; i < n; i++)
        if (transcripts[i].buflen >= kKeccakRate) return ZIP_ERR_INVALID_PARAM;
    if (device < 0 || device >= kMaxDevices) return ZIP_ERR_NO_DEVICE;
    PrimeDev &pd = g_prime[device];
    std::lock_guard<std::mutex> g(pd.mu);
    CurrentDeviceGuard restore;
    if (int32_t rc = prime_dev_ready(pd, device)) return rc;
    // (per call: the tests flip it)
    const uint32_t w = prime_batch_knob(getenv("ZIP_HIP_PRIME_BATCH_WINDOW"), kPrimeBatchDefaultWindow, kPrimeBatchMaxWindow);
    return with_fl(limbs, [&](auto FL) {
        return get_prime_batch_fl<decltype(FL)::value>(pd, transcripts, n, w, primes_out, candidates_tried_out);
    });
}

void zip_prime_batch_counts(uint64_t *calls, uint64_t *members, uint64_t *kernel_launches) {
    if (calls) *calls = g_prime_batch_calls.load();
    if (members) *members = g_prime_batch_members.load();
    if (kernel_launches) *kernel_launches = g_prime_batch_launches.load();
}

const char *zip_sumcheck_last_error(const zip_sumcheck *s) { return s && s->ctx ? s->ctx->last_error.c_str() : ""; }

void zip_sumcheck_free(zip_sumcheck *s) {
    if (!s) return;
    if (s->ctx) {
        if (s->ctx->stream) (void)stream_wait(s->ctx->stream);
        slab_give(s->ctx->device, s->evals_pinned);
        if (!s->owned) {  // the caller's tables are not ours to free
            std::lock_guard<std::mutex> g(s->ctx->mu);
            for (auto *p : s->input) s->ctx->live_blocks.erase(const_cast<uint64_t *>(p));
        }
        zip_ctx_destroy(s->ctx);  // frees every pool block, the stream, the events
    }
    delete s;
}

// ---------------------------------------------------------------------------- zip_ccs
namespace {
// the ranges of t and s, then the shape rules of the t matrices of a CCS with m = 2^s columns (zip_ccs_create,
// zip_ccs_batch_create)
int32_t ccs_check_matrices(const zip_sparse_matrix *mats, uint32_t t, uint32_t s) {
    if (t < 1 || t > (uint32_t)kCcsMaxMatrices || s < 1 || s > 28) return ZIP_ERR_INVALID_PARAM;
    const uint32_t m = 1u << s;
    for (uint32_t k = 0; k < t; k++) {
        const zip_sparse_matrix &M = mats[k];
        if (!M.row_ptr || (M.row_ptr[M.n_rows] && (!M.col_idx || !M.values))) return ZIP_ERR_NULL;
        // mat_vec_mul: "M.n_cols != z.len()" (ccs/utils.rs:52-59); more rows than 2^s: to_mles_err (zinc/utils.rs:150)
        if (M.n_cols != m || M.n_rows > m) return ZIP_ERR_SHAPE;
        if (M.row_ptr[0] != 0) return ZIP_ERR_INVALID_PARAM;
        for (uint32_t r = 0; r < M.n_rows; r++)
            if (M.row_ptr[r + 1] < M.row_ptr[r]) return ZIP_ERR_INVALID_PARAM;
        for (uint32_t e = 0; e < M.row_ptr[M.n_rows]; e++)
            if (M.col_idx[e] >= m) return ZIP_ERR_SHAPE;  // the reference indexes out of bounds (panic)
    }
    return ZIP_OK;
}

// One matrix of m columns into the pool, up to its transposition: the arrays of D (values of `val_bytes` each, not
// filled here), the CSR indices uploaded, col_ptr counted and scanned, and a copy of it in *cursor (the per-column write
// positions of csc_fill_kernel).  The caller uploads D.vals, launches csc_fill_kernel, and releases *cursor and *sums
// once the stream has passed them.
int32_t ccs_upload_matrix(zip_ctx *ctx, const zip_sparse_matrix &M, uint32_t m, size_t val_bytes, zip_ccs::Mat &D, uint32_t **cursor,
                          uint32_t **sums) {
    const uint32_t nnz = M.row_ptr[M.n_rows], n_cnt = m + 1, tiles = (n_cnt + kScanTile - 1) / kScanTile;
    D.n_rows = M.n_rows;
    D.nnz = nnz;
    int32_t rc;
    if ((rc = pool_alloc(ctx, (size_t)(M.n_rows + 1) * 4, (void **)&D.row_ptr))) return rc;
    if ((rc = pool_alloc(ctx, (size_t)nnz * 4, (void **)&D.col_idx))) return rc;
    if ((rc = pool_alloc(ctx, (size_t)n_cnt * 4, (void **)&D.col_ptr))) return rc;
    if ((rc = pool_alloc(ctx, (size_t)nnz * 4, (void **)&D.row_idx))) return rc;
    if ((rc = pool_alloc(ctx, (size_t)nnz * val_bytes, (void **)&D.vals))) return rc;
    if ((rc = pool_alloc(ctx, (size_t)nnz * val_bytes, (void **)&D.vals_t))) return rc;
    if ((rc = pool_alloc(ctx, (size_t)n_cnt * 4, (void **)cursor))) return rc;
    if ((rc = pool_alloc(ctx, (size_t)tiles * 4, (void **)sums))) return rc;
    if ((rc = copy_h2d_bounced(ctx, D.row_ptr, M.row_ptr, (size_t)(M.n_rows + 1) * 4, ctx->stream))) return rc;
    if (hipMemsetAsync(D.col_ptr, 0, (size_t)n_cnt * 4, ctx->stream) != hipSuccess) return ZIP_ERR_HIP;
    if (nnz) {
        if ((rc = copy_h2d_bounced(ctx, D.col_idx, M.col_idx, (size_t)nnz * 4, ctx->stream))) return rc;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)nnz + 255) / 256, 65535);
        hipLaunchKernelGGL(csc_count_kernel, dim3(blocks), dim3(256), 0, ctx->stream, D.col_idx, nnz, D.col_ptr);
    }
    // col_ptr = inclusive scan of the counters (counts sit at [col + 1], so col_ptr[0] = 0)
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(tiles), dim3(kScanBlock), 0, ctx->stream, D.col_ptr, n_cnt, *sums,
                       static_cast<const uint32_t *>(nullptr));
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kScanBlock), 0, ctx->stream, *sums, tiles);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(tiles), dim3(kScanBlock), 0, ctx->stream, D.col_ptr, n_cnt,
                       static_cast<uint32_t *>(nullptr), static_cast<const uint32_t *>(*sums));
    if (hipMemcpyAsync(*cursor, D.col_ptr, (size_t)n_cnt * 4, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return ZIP_ERR_HIP;
    return ZIP_OK;
}
}  // namespace

int32_t zip_ccs_create(int32_t device, const zip_sparse_matrix *mats, uint32_t t, uint32_t s, const zip_field *field,
                       zip_ccs **out) {
    if (!mats || !out || !field) return ZIP_ERR_NULL;
    *out = nullptr;
    if (int32_t rc = ccs_check_matrices(mats, t, s)) return rc;
    const uint32_t m = 1u << s;
    zip_ctx *ctx = nullptr;
    int32_t rc = private_ctx_create(device, true, &ctx);
    if (rc) return rc;
    zip_ccs *c = new (std::nothrow) zip_ccs();
    if (!c) { zip_ctx_destroy(ctx); return ZIP_ERR_ALLOC; }
    ctx->h2d_bounce_threshold = (size_t)256 << 10;  // MiB-sized index arrays: staged pageable copies run at 3-4 GB/s
    c->ctx = ctx;
    do {
        HostField &hf = c->field;
        if ((rc = make_field(ctx, field, &hf))) break;
        c->t = t;
        c->s = s;
        c->m = m;
        c->fl = hf.fl;
        const size_t elem = (size_t)hf.fl * 8, tab = (size_t)m * elem;
        for (uint32_t k = 0; k < t && rc == ZIP_OK; k++) {
            const zip_sparse_matrix &M = mats[k];
            zip_ccs::Mat &D = c->mat[k];
            void *tmp = nullptr;
            uint32_t *cursor = nullptr, *sums = nullptr;
            if ((rc = ccs_upload_matrix(ctx, M, m, elem, D, &cursor, &sums))) break;
            if (D.nnz) {
                if ((rc = pool_alloc(ctx, (size_t)D.nnz * 8, &tmp))) break;  // i64 values before the field map
                // SparseMatrix::map_to_field (sparse_matrix.rs:38-58)
                if ((rc = copy_h2d_bounced(ctx, tmp, M.values, (size_t)D.nnz * 8, ctx->stream))) break;
                rc = with_fl(hf.fl, [&](auto FL) { return ccs_map_i64<decltype(FL)::value>(ctx, static_cast<const int64_t *>(tmp), D.nnz, D.nnz, D.vals, hf); });
                if (rc) break;
                const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)M.n_rows + 255) / 256, 65535);
                with_fl(hf.fl, [&](auto FL) {
                    hipLaunchKernelGGL(csc_fill_kernel<decltype(FL)::value>, dim3(blocks), dim3(256), 0, ctx->stream, D.row_ptr, D.col_idx, D.vals, M.n_rows, cursor, D.row_idx, D.vals_t);
                });
            }
            if (hipGetLastError() != hipSuccess || stream_wait(ctx->stream) != hipSuccess) { rc = ZIP_ERR_HIP; break; }
            pool_release(ctx, tmp);
            pool_release(ctx, cursor);
            pool_release(ctx, sums);
            if ((rc = pool_alloc(ctx, tab, (void **)&c->mz[k]))) break;
        }
        if (rc) break;
        if ((rc = pool_alloc(ctx, tab, (void **)&c->z_f))) break;
        if ((rc = pool_alloc(ctx, tab, (void **)&c->eq[0]))) break;
        if ((rc = pool_alloc(ctx, tab, (void **)&c->eq[1]))) break;
        if ((rc = pool_alloc(ctx, tab, (void **)&c->second))) break;
        if ((rc = pool_alloc(ctx, (size_t)(40 + kCcsMaxMatrices) * 64, (void **)&c->small_d))) break;
        if ((rc = pool_alloc(ctx, (((size_t)1 << (s / 2)) + ((size_t)1 << (s - s / 2))) * elem, (void **)&c->eq_half))) break;
        c->dot_blocks = (uint32_t)std::min<uint64_t>(((uint64_t)m + 255) / 256, (uint64_t)ctx->num_cus * 4);
        if ((rc = pool_alloc(ctx, (size_t)c->dot_blocks * elem, (void **)&c->partials))) break;
    } while (0);
    if (rc) {
        zip_ccs_free(c);
        return rc;
    }
    *out = c;
    return ZIP_OK;
}

void zip_ccs_free(zip_ccs *c) {
    if (!c) return;
    if (c->ctx) zip_ctx_destroy(c->ctx);  // frees every pool block and the stream
    delete c;
}

const char *zip_ccs_last_error(const zip_ccs *c) { return c && c->ctx ? c->ctx->last_error.c_str() : ""; }

int32_t zip_ccs_set_z(zip_ccs *c, const int64_t *z, size_t z_len, zip_mem_kind kind) {
    if (!c || (!z && z_len)) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (z_len > c->m) return fail(ctx, ZIP_ERR_SHAPE, "z has %zu entries, the matrices %u columns", z_len, c->m);
    const HostField &hf = c->field;
    int32_t rc;
    Scratch in(ctx);
    const int64_t *z_d = z;
    if (kind == ZIP_MEM_HOST && z_len) {
        if ((rc = in.get(z_len * 8))) return rc;
        if ((rc = copy_h2d_bounced(ctx, in.ptr, z, z_len * 8, ctx->stream))) return rc;
        z_d = in.as<int64_t>();
    }
    if ((rc = with_fl(c->fl, [&](auto FL) { return ccs_set_z_fl<decltype(FL)::value>(c, z_d, z_len, hf); }))) return rc;
    HIP_TRY(ctx, stream_wait(ctx->stream));
    c->have_z = true;
    c->have_second = false;
    return ZIP_OK;
}

int32_t zip_ccs_eq_table(zip_ccs *c, const uint64_t *r, uint32_t slot) {
    if (!c || !r) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (slot > 1) return fail(ctx, ZIP_ERR_INVALID_PARAM, "slot %u: 0 = eq(beta), 1 = eq(r_x)", slot);
    const HostField &hf = c->field;
    int32_t rc;
    HIP_TRY(ctx, hipMemcpyAsync(c->small_d, r, (size_t)c->s * c->fl * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = with_fl(c->fl, [&](auto FL) { return ccs_eq_table_fl<decltype(FL)::value>(c, c->small_d, slot, hf); }))) return rc;
    HIP_TRY(ctx, stream_wait(ctx->stream));
    c->have_eq[slot] = true;
    return ZIP_OK;
}

int32_t zip_ccs_second_table(zip_ccs *c, const uint64_t *r_x, const uint64_t *gamma, uint64_t *v_s_out) {
    if (!c || !r_x || !gamma || !v_s_out) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (!c->have_z) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_ccs_set_z has not run");
    int32_t rc;
    if ((rc = zip_ccs_eq_table(c, r_x, 1))) return rc;
    const HostField &hf = c->field;
    uint64_t *gamma_d = c->small_d + (size_t)32 * 8, *vs_d = c->small_d + (size_t)33 * 8;
    HIP_TRY(ctx, hipMemcpyAsync(gamma_d, gamma, (size_t)c->fl * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = with_fl(c->fl, [&](auto FL) { return ccs_second_fl<decltype(FL)::value>(c, gamma_d, vs_d, hf); }))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(v_s_out, vs_d, (size_t)c->t * c->fl * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    c->have_second = true;
    return ZIP_OK;
}

int32_t zip_ccs_eval_matrices(zip_ccs *c, const uint64_t *r_x, const uint64_t *r_y, uint64_t *v_xy_out) {
    if (!c || !r_x || !r_y || !v_xy_out) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    int32_t rc;
    if ((rc = zip_ccs_eq_table(c, r_x, 0))) return rc;  // both eq slots are overwritten
    if ((rc = zip_ccs_eq_table(c, r_y, 1))) return rc;
    c->have_second = false;
    const HostField &hf = c->field;
    uint64_t *out_d = c->small_d + (size_t)33 * 8;
    if ((rc = with_fl(c->fl, [&](auto FL) { return ccs_eval_matrices_fl<decltype(FL)::value>(c, out_d, hf); }))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(v_xy_out, out_d, (size_t)c->t * c->fl * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, stream_wait(ctx->stream));
    return ZIP_OK;
}

int32_t zip_ccs_table(zip_ccs *c, zip_ccs_table_kind which, uint32_t index, const uint64_t **table_dev) {
    if (!c || !table_dev) return ZIP_ERR_NULL;
    zip_ctx *ctx = c->ctx;
    *table_dev = nullptr;
    switch (which) {
        case ZIP_CCS_Z_FIELD:
            if (!c->have_z) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_ccs_set_z has not run");
            *table_dev = c->z_f;
            return ZIP_OK;
        case ZIP_CCS_MZ:
            if (!c->have_z) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_ccs_set_z has not run");
            if (index >= c->t) return fail(ctx, ZIP_ERR_INVALID_PARAM, "matrix %u of %u", index, c->t);
            *table_dev = c->mz[index];
            return ZIP_OK;
        case ZIP_CCS_EQ:
            if (index > 1 || !c->have_eq[index]) return fail(ctx, ZIP_ERR_INVALID_PARAM, "eq table %u has not been built", index);
            *table_dev = c->eq[index];
            return ZIP_OK;
        case ZIP_CCS_SECOND:
            if (!c->have_second) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_ccs_second_table has not run");
            *table_dev = c->second;
            return ZIP_OK;
    }
    return fail(ctx, ZIP_ERR_INVALID_PARAM, "unknown table kind %d", (int)which);
}

int32_t zip_ccs_download(zip_ccs *c, zip_ccs_table_kind which, uint32_t index, uint64_t *out) {
    if (!c || !out) return ZIP_ERR_NULL;
    const uint64_t *d = nullptr;
    int32_t rc = zip_ccs_table(c, which, index, &d);
    if (rc) return rc;
    zip_ctx *ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return copy_d2h_bounced(ctx, out, d, (size_t)c->m * c->fl * 8, ctx->stream);
}

// ---------------------------------------------------------------------------- zip_ccs_batch
int32_t zip_ccs_batch_create(int32_t device, const zip_sparse_matrix *mats, uint32_t t, uint32_t s, uint32_t limbs,
                             uint32_t capacity, zip_ccs_batch **out) {
    // usage errors, before a device is looked for: NULLs, the ranges, the matrices, then this entry point's own size limit
    if (!mats || !out) return ZIP_ERR_NULL;
    *out = nullptr;
    if (limbs < 2 || limbs > 4 || capacity < 1 || capacity > 65535) return ZIP_ERR_INVALID_PARAM;
    if (int32_t rc = ccs_check_matrices(mats, t, s)) return rc;  // (zip_ccs_create's ranges and rules)
    if (s > kCcsBatchMaxVars) return ZIP_ERR_UNSUPPORTED;
    static_assert(kCcsBatchMaxVars == kBatchSumcheckMaxVars, "the tables feed zip_sumcheck_prove_batch");
    const uint32_t m = 1u << s;
    zip_ctx *ctx = nullptr;
    int32_t rc = private_ctx_create(device, true, &ctx);
    if (rc) return rc;
    const size_t elem = (size_t)limbs * 8, tab = (size_t)m * elem;
    const size_t tables_bytes = (size_t)capacity * (t + 4) * tab, z_bytes = (size_t)capacity * m * 8;
    {   // what cannot fit is refused without asking the allocator for it
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) rc = ZIP_ERR_HIP;
        else if (tables_bytes + z_bytes > total_b) rc = ZIP_ERR_ALLOC;
    }
    zip_ccs_batch *b = rc ? nullptr : new (std::nothrow) zip_ccs_batch();
    if (!b) { zip_ctx_destroy(ctx); return rc ? rc : ZIP_ERR_ALLOC; }
    ctx->h2d_bounce_threshold = (size_t)256 << 10;  // (as zip_ccs_create)
    b->ctx = ctx;
    b->t = t;
    b->s = s;
    b->m = m;
    b->fl = limbs;
    b->capacity = capacity;
    b->mats.t = t;
    b->mats.m = m;
    do {
        std::vector<void *> tmp;  // per-matrix cursors and tile sums: released once the stream has passed them
        for (uint32_t k = 0; k < t && rc == ZIP_OK; k++) {
            const zip_sparse_matrix &M = mats[k];
            zip_ccs::Mat D;
            uint32_t *cursor = nullptr, *sums = nullptr;
            if ((rc = ccs_upload_matrix(ctx, M, m, 8, D, &cursor, &sums))) break;
            tmp.push_back(cursor);
            tmp.push_back(sums);
            b->mats.row_ptr[k] = D.row_ptr;
            b->mats.col_idx[k] = D.col_idx;
            b->mats.vals[k] = reinterpret_cast<const int64_t *>(D.vals);
            b->mats.col_ptr[k] = D.col_ptr;
            b->mats.row_idx[k] = D.row_idx;
            b->mats.vals_t[k] = reinterpret_cast<const int64_t *>(D.vals_t);
            b->mats.n_rows[k] = M.n_rows;
            if (D.nnz) {  // the int64 values travel as one-limb elements
                if ((rc = copy_h2d_bounced(ctx, D.vals, M.values, (size_t)D.nnz * 8, ctx->stream))) break;
                const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)M.n_rows + 255) / 256, 65535);
                hipLaunchKernelGGL(csc_fill_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, D.row_ptr, D.col_idx, D.vals, M.n_rows, cursor,
                                   D.row_idx, D.vals_t);
            }
            if (hipGetLastError() != hipSuccess) { rc = ZIP_ERR_HIP; break; }
        }
        if (rc) break;
        if ((rc = pool_alloc(ctx, tables_bytes, (void **)&b->tables))) break;
        if ((rc = pool_alloc(ctx, z_bytes, (void **)&b->z_d))) break;
        const size_t inst_bytes = with_fl(limbs, [](auto FL) { return sizeof(CcsBatchInst<decltype(FL)::value>); });
        // (behind the entries: room for the two points per instance that zip_ccs_batch_eval_matrices uploads with them)
        if ((rc = pool_alloc(ctx, (size_t)capacity * (inst_bytes + 2 * s * elem), &b->args_d))) break;
        if ((rc = pool_alloc(ctx, (size_t)capacity * (s + 1) * elem, (void **)&b->chal_d))) break;
        if ((rc = pool_alloc(ctx, (size_t)capacity * t * elem, (void **)&b->vs_d))) break;
        if (stream_wait(ctx->stream) != hipSuccess) { rc = ZIP_ERR_HIP; break; }  // ONE wait for all t transpositions
        for (void *p : tmp) pool_release(ctx, p);
    } while (0);
    if (rc) {
        zip_ccs_batch_free(b);
        return rc;
    }
    *out = b;
    return ZIP_OK;
}

void zip_ccs_batch_free(zip_ccs_batch *b) {
    if (!b) return;
    if (b->ctx) {
        if (b->ctx->stream) (void)stream_wait(b->ctx->stream);  // the staging vectors die with the handle
        zip_ctx_destroy(b->ctx);  // frees every pool block and the stream
    }
    delete b;
}

const char *zip_ccs_batch_last_error(const zip_ccs_batch *b) { return b && b->ctx ? b->ctx->last_error.c_str() : ""; }

int32_t zip_ccs_batch_set_z(zip_ccs_batch *b, const zip_field *const *fields, const int64_t *const *z, const size_t *z_len,
                            uint32_t n, zip_mem_kind kind) {
    // usage errors, before anything reaches the device: every NULL, then n, the fields, then the lengths
    if (!b || !fields || !z || !z_len) return ZIP_ERR_NULL;
    zip_ctx *ctx = b->ctx;
    const uint32_t scan = std::min(n, b->capacity);
    for (uint32_t i = 0; i < scan; i++)
        if (!fields[i] || (!z[i] && z_len[i])) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (n < 1 || n > b->capacity) return fail(ctx, ZIP_ERR_INVALID_PARAM, "%u instances, the handle was made for 1..%u", n, b->capacity);
    for (uint32_t i = 0; i < n; i++)
        if (fields[i]->limbs != b->fl)
            return fail(ctx, ZIP_ERR_INVALID_PARAM, "instance %u: a field of %u limbs, the handle was made for %u", i, fields[i]->limbs, b->fl);
    // FieldConfig::new per instance (an even modulus or 1: ZIP_ERR_INVALID_PARAM); neighbours with the same modulus share the work
    std::vector<HostField> hf(n);
    for (uint32_t i = 0; i < n; i++) {
        if (i && !memcmp(fields[i]->modulus, fields[i - 1]->modulus, 8 * (size_t)b->fl)) {
            hf[i] = hf[i - 1];
            continue;
        }
        if (int32_t rc = make_field_uncached(ctx, fields[i], &hf[i])) return rc;
    }
    for (uint32_t i = 0; i < n; i++)
        if (z_len[i] > b->m) return fail(ctx, ZIP_ERR_SHAPE, "instance %u: z has %zu entries, the matrices %u columns", i, z_len[i], b->m);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = ccs_batch_wait(b))) return rc;  // the staging vectors of the previous call
    b->n = 0;  // (a call that fails from here on leaves no tables)
    b->have_eq[0] = b->have_eq[1] = b->have_second = false;
    std::vector<const int64_t *> z_dev(n);
    if (kind == ZIP_MEM_HOST) {  // one gathered copy for all z
        size_t total = 0;
        for (uint32_t i = 0; i < n; i++) total += z_len[i];
        b->z_h.resize(total);
        for (size_t i = 0, at = 0; i < n; at += z_len[i], i++) {
            if (z_len[i]) memcpy(b->z_h.data() + at, z[i], z_len[i] * 8);
            z_dev[i] = b->z_d + at;
        }
        b->in_flight = true;
        if (total && (rc = copy_h2d_bounced(ctx, b->z_d, b->z_h.data(), total * 8, ctx->stream))) return rc;
    } else {
        for (uint32_t i = 0; i < n; i++) z_dev[i] = z[i];
    }
    with_fl(b->fl, [&](auto FL) { ccs_batch_fill_args<decltype(FL)::value>(b, hf, z_dev, z_len, n); });
    b->in_flight = true;
    HIP_TRY(ctx, hipMemcpyAsync(b->args_d, b->args_h.data(), b->args_h.size(), hipMemcpyHostToDevice, ctx->stream));
    b->n = n;
    if ((rc = with_fl(b->fl, [&](auto FL) { return ccs_batch_set_z_fl<decltype(FL)::value>(b); }))) {
        b->n = 0;
        return rc;
    }
    g_ccs_batch_instances += n;
    return ZIP_OK;
}

int32_t zip_ccs_batch_eq_tables(zip_ccs_batch *b, const uint64_t *r, uint32_t slot) {
    if (!b || !r) return ZIP_ERR_NULL;
    zip_ctx *ctx = b->ctx;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (slot > 1) return fail(ctx, ZIP_ERR_INVALID_PARAM, "slot %u: 0 = eq(beta), 1 = eq(r_x)", slot);
    if (!b->n) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_ccs_batch_set_z has not run");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = ccs_batch_wait(b))) return rc;  // (chal_h may still be on its way up)
    const size_t words = (size_t)b->n * b->s * b->fl;
    b->chal_h.assign(r, r + words);
    b->in_flight = true;
    HIP_TRY(ctx, hipMemcpyAsync(b->chal_d, b->chal_h.data(), words * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = with_fl(b->fl, [&](auto FL) { return ccs_batch_eq_fl<decltype(FL)::value>(b, b->chal_d, slot); }))) return rc;
    b->have_eq[slot] = true;
    if (slot == 1) b->have_second = false;
    return ZIP_OK;
}

int32_t zip_ccs_batch_second_tables(zip_ccs_batch *b, const uint64_t *r_x, const uint64_t *gamma, uint64_t *v_s_out) {
    if (!b || !r_x || !gamma || !v_s_out) return ZIP_ERR_NULL;
    zip_ctx *ctx = b->ctx;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (!b->n) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_ccs_batch_set_z has not run");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = ccs_batch_wait(b))) return rc;
    // one upload: every r_x, then every gamma
    const size_t r_words = (size_t)b->n * b->s * b->fl, g_words = (size_t)b->n * b->fl;
    b->chal_h.assign(r_x, r_x + r_words);
    b->chal_h.insert(b->chal_h.end(), gamma, gamma + g_words);
    b->in_flight = true;
    b->have_second = false;
    HIP_TRY(ctx, hipMemcpyAsync(b->chal_d, b->chal_h.data(), (r_words + g_words) * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = with_fl(b->fl, [&](auto FL) { return ccs_batch_eq_fl<decltype(FL)::value>(b, b->chal_d, 1); }))) return rc;
    if ((rc = with_fl(b->fl, [&](auto FL) { return ccs_batch_second_fl<decltype(FL)::value>(b, b->chal_d + r_words); }))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(v_s_out, b->vs_d, (size_t)b->n * b->t * b->fl * 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ccs_batch_wait(b))) return rc;
    b->have_eq[1] = b->have_second = true;
    return ZIP_OK;
}

int32_t zip_ccs_batch_table(zip_ccs_batch *b, uint32_t instance, zip_ccs_table_kind which, uint32_t index,
                            const uint64_t **table_dev) {
    if (!b || !table_dev) return ZIP_ERR_NULL;
    zip_ctx *ctx = b->ctx;
    *table_dev = nullptr;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (!b->n) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_ccs_batch_set_z has not run");
    if (instance >= b->n) return fail(ctx, ZIP_ERR_INVALID_PARAM, "instance %u of %u", instance, b->n);
    uint32_t j = 0;
    switch (which) {
        case ZIP_CCS_Z_FIELD:
            break;
        case ZIP_CCS_MZ:
            if (index >= b->t) return fail(ctx, ZIP_ERR_INVALID_PARAM, "matrix %u of %u", index, b->t);
            j = 1 + index;
            break;
        case ZIP_CCS_EQ:
            if (index > 1 || !b->have_eq[index]) return fail(ctx, ZIP_ERR_INVALID_PARAM, "eq table %u has not been built", index);
            j = b->t + 1 + index;
            break;
        case ZIP_CCS_SECOND:
            if (!b->have_second) return fail(ctx, ZIP_ERR_INVALID_PARAM, "zip_ccs_batch_second_tables has not run");
            j = b->t + 3;
            break;
        default:
            return fail(ctx, ZIP_ERR_INVALID_PARAM, "unknown table kind %d", (int)which);
    }
    // the tables are read by other streams (zip_sumcheck_prove_batch has its own): complete before the pointer leaves
    if (b->in_flight) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (int32_t rc = ccs_batch_wait(b)) return rc;
    }
    *table_dev = ccs_batch_table_at(b, instance, j);
    return ZIP_OK;
}

int32_t zip_ccs_batch_download(zip_ccs_batch *b, uint32_t instance, zip_ccs_table_kind which, uint32_t index, uint64_t *out) {
    if (!b || !out) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(b->ctx->api_mu);
    const uint64_t *d = nullptr;
    int32_t rc = zip_ccs_batch_table(b, instance, which, index, &d);
    if (rc) return rc;
    zip_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return copy_d2h_bounced(ctx, out, d, (size_t)b->m * b->fl * 8, ctx->stream);
}

int32_t zip_ccs_batch_eval_matrices(zip_ccs_batch *b, const zip_field *const *fields, uint32_t n, const uint64_t *r_x,
                                    const uint64_t *r_y, uint64_t *v_xy_out) {
    // usage errors, before anything reaches the device, in set_z's order: every NULL, then n, then the fields
    if (!b || !fields || !r_x || !r_y || !v_xy_out) return ZIP_ERR_NULL;
    zip_ctx *ctx = b->ctx;
    const uint32_t scan = std::min(n, b->capacity);
    for (uint32_t i = 0; i < scan; i++)
        if (!fields[i]) return ZIP_ERR_NULL;
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (n < 1 || n > b->capacity) return fail(ctx, ZIP_ERR_INVALID_PARAM, "%u instances, the handle was made for 1..%u", n, b->capacity);
    for (uint32_t i = 0; i < n; i++)
        if (fields[i]->limbs != b->fl)
            return fail(ctx, ZIP_ERR_INVALID_PARAM, "instance %u: a field of %u limbs, the handle was made for %u", i, fields[i]->limbs, b->fl);
    std::vector<HostField> hf(n);
    for (uint32_t i = 0; i < n; i++) {
        if (i && !memcmp(fields[i]->modulus, fields[i - 1]->modulus, 8 * (size_t)b->fl)) {
            hf[i] = hf[i - 1];
            continue;
        }
        if (int32_t rc = make_field_uncached(ctx, fields[i], &hf[i])) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    if ((rc = ccs_batch_wait(b))) return rc;  // the staging vectors of the previous call
    // the instances of a previous set_z are replaced: the table calls answer ZIP_ERR_INVALID_PARAM until the next one
    b->n = 0;
    b->have_eq[0] = b->have_eq[1] = b->have_second = false;
    const std::vector<const int64_t *> no_z(n, nullptr);
    const std::vector<size_t> no_len(n, 0);
    with_fl(b->fl, [&](auto FL) { ccs_batch_fill_args<decltype(FL)::value>(b, hf, no_z, no_len.data(), n); });
    // one upload: the entries, every r_x, every r_y
    const size_t inst_bytes = b->args_h.size(), r_words = (size_t)n * b->s * b->fl;
    b->args_h.resize(inst_bytes + 2 * r_words * 8);
    memcpy(b->args_h.data() + inst_bytes, r_x, r_words * 8);
    memcpy(b->args_h.data() + inst_bytes + r_words * 8, r_y, r_words * 8);
    b->in_flight = true;
    HIP_TRY(ctx, hipMemcpyAsync(b->args_d, b->args_h.data(), b->args_h.size(), hipMemcpyHostToDevice, ctx->stream));
    const uint64_t *r_d = reinterpret_cast<const uint64_t *>(static_cast<const unsigned char *>(b->args_d) + inst_bytes);
    b->n = n;  // (the launchers size their grids by it)
    rc = with_fl(b->fl, [&](auto FL) {
        constexpr int L = decltype(FL)::value;
        int32_t r = ccs_batch_eq_fl<L>(b, r_d, 0);
        if (!r) r = ccs_batch_eq_fl<L>(b, r_d + r_words, 1);
        if (!r) r = ccs_batch_eval_matrices_fl<L>(b);
        return r;
    });
    b->n = 0;
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(v_xy_out, b->vs_d, (size_t)n * b->t * b->fl * 8, hipMemcpyDeviceToHost, ctx->stream));
    return ccs_batch_wait(b);
}

void zip_ccs_batch_counts(uint64_t *kernel_launches, uint64_t *instances) {
    if (kernel_launches) *kernel_launches = g_ccs_batch_launches.load();
    if (instances) *instances = g_ccs_batch_instances.load();
}

int32_t zip_sum_partials(zip_ctx *ctx, const uint64_t *uparts, const uint64_t *fparts, uint32_t n_parts,
                         const zip_field *field, uint64_t *uprime_out, uint64_t *row_out) {
    if (!ctx) return ZIP_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (int32_t r = refuse_two_limb(ctx, "zip_sum_partials")) return r;  // (the partials of row shards, which such a ctx has not)
    if ((uparts && !uprime_out) || (fparts && !row_out)) return ZIP_ERR_NULL;
    HostField hf;
    hf.fl = 4;
    int32_t rc;
    if (fparts && (rc = make_field(ctx, field, &hf))) return rc;
    const uint32_t C = ctx->p.row_len;
    const dim3 grid((C + 255) / 256), block(256);
    LaunchTimer t(ctx, "sum_partials_kernel");
    with_fl(hf.fl, [&](auto FL) {
        constexpr int N = decltype(FL)::value;
        hipLaunchKernelGGL(sum_partials_kernel<N>, grid, block, 0, ctx->stream, uparts, fparts, n_parts, C,
                           ctx->p.m_limbs, uprime_out, row_out, to_dev<N>(hf));
    });
    HIP_TRY(ctx, hipGetLastError());
    return ZIP_OK;
}

int32_t zip_merkle_trees(int32_t device, const uint64_t *leaves, uint32_t leaf_limbs, uint32_t depth,
                         uint32_t num_trees, zip_mem_kind kind, uint8_t *layers_out) {
    if (!leaves || !layers_out) return ZIP_ERR_NULL;
    if (leaf_limbs < 1 || leaf_limbs > 8 || depth > 24 || num_trees == 0) return ZIP_ERR_INVALID_PARAM;
    // a throw-away ctx gives us the stream / pool / error plumbing
    zip_ctx *ctx = nullptr;
    int32_t rc = private_ctx_create(device, false, &ctx);
    if (rc) return rc;
    const uint32_t n = 1u << depth;
    const size_t leaf_bytes = (size_t)num_trees * n * leaf_limbs * 8;
    const size_t tree_bytes = (size_t)num_trees * 2 * n * 32;
    const size_t out_w = ((size_t)2 * n - 1) * 32;
    void *leaves_d = nullptr, *layers_d = nullptr, *roots_d = nullptr;
    do {
        if (kind == ZIP_MEM_HOST) {
            if ((rc = pool_alloc(ctx, leaf_bytes, &leaves_d))) break;
            if (hipMemcpyAsync(leaves_d, leaves, leaf_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = ZIP_ERR_HIP; break; }
        } else {
            leaves_d = const_cast<uint64_t *>(leaves);
        }
        if ((rc = pool_alloc(ctx, tree_bytes, &layers_d))) break;
        if ((rc = pool_alloc(ctx, (size_t)num_trees * 32, &roots_d))) break;
        const size_t total = (size_t)num_trees * n;
        const dim3 grid((uint32_t)((total + 255) / 256)), block(256);
        const uint64_t *L = static_cast<const uint64_t *>(leaves_d);
        uint32_t *Y = static_cast<uint32_t *>(layers_d);
        switch (leaf_limbs) {
            case 1: hipLaunchKernelGGL(merkle_leaves_kernel<1>, grid, block, 0, ctx->stream, L, Y, num_trees, n); break;
            case 2: hipLaunchKernelGGL(merkle_leaves_kernel<2>, grid, block, 0, ctx->stream, L, Y, num_trees, n); break;
            case 3: hipLaunchKernelGGL(merkle_leaves_kernel<3>, grid, block, 0, ctx->stream, L, Y, num_trees, n); break;
            case 4: hipLaunchKernelGGL(merkle_leaves_kernel<4>, grid, block, 0, ctx->stream, L, Y, num_trees, n); break;
            case 5: hipLaunchKernelGGL(merkle_leaves_kernel<5>, grid, block, 0, ctx->stream, L, Y, num_trees, n); break;
            case 6: hipLaunchKernelGGL(merkle_leaves_kernel<6>, grid, block, 0, ctx->stream, L, Y, num_trees, n); break;
            case 7: hipLaunchKernelGGL(merkle_leaves_kernel<7>, grid, block, 0, ctx->stream, L, Y, num_trees, n); break;
            default: hipLaunchKernelGGL(merkle_leaves_kernel<8>, grid, block, 0, ctx->stream, L, Y, num_trees, n); break;
        }
        if (hipGetLastError() != hipSuccess) { rc = ZIP_ERR_HIP; break; }
        if ((rc = merkle_upper_levels(ctx, ctx->stream, Y, static_cast<uint32_t *>(roots_d), num_trees, n, 0, depth))) break;
        hipError_t e = hipMemcpy2DAsync(layers_out, out_w, layers_d, (size_t)2 * n * 32, out_w, num_trees,
                                        kind == ZIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                        ctx->stream);
        if (e == hipSuccess) e = stream_wait(ctx->stream);
        if (e != hipSuccess) rc = ZIP_ERR_HIP;
    } while (0);
    if (kind != ZIP_MEM_HOST) {
        std::lock_guard<std::mutex> g(ctx->mu);
        ctx->live_blocks.erase(leaves_d);  // not ours
    }
    zip_ctx_destroy(ctx);
    return rc;
}

int32_t zip_ctx_set_profiling(zip_ctx *ctx, int32_t on) {
    if (!ctx) return ZIP_ERR_NULL;
    ctx->profiling = on != 0;
    ctx->profile_commit_only = on == 2;
    return ZIP_OK;
}

int32_t zip_ctx_commit_clock(zip_ctx *ctx, double *mhz_out) {
    if (!ctx || !mhz_out) return ZIP_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    if (ctx->s_commit) HIP_TRY(ctx, stream_wait(ctx->s_commit));
    const unsigned long long *c = ctx->clock_h;
    *mhz_out = (c && c[3] > c[1] && c[2] > c[0]) ? (double)(c[2] - c[0]) / (double)(c[3] - c[1]) * 100.0 : 0.0;
    return ZIP_OK;
}

int32_t zip_ctx_profile_read(zip_ctx *ctx, zip_kernel_time *out, uint32_t cap) {
    if (!ctx) return ZIP_ERR_NULL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::recursive_mutex> api_lock(ctx->api_mu);
    HIP_TRY(ctx, stream_wait(ctx->stream));
    for (auto &pe : ctx->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pe.start, pe.stop) == hipSuccess) {
            KernelStat &s = ctx->stats[pe.name];
            s.launches++;
            s.total_ms += ms;
        }
        ctx->event_pool.push_back(pe.start);
        ctx->event_pool.push_back(pe.stop);
    }
    ctx->pending.clear();
    ctx->stat_names.clear();
    ctx->stat_names.reserve(ctx->stats.size());
    uint32_t n = 0;
    for (auto &kv : ctx->stats) {
        ctx->stat_names.push_back(kv.first);
        if (out && n < cap) {
            out[n].name = ctx->stat_names.back().c_str();
            out[n].launches = kv.second.launches;
            out[n].total_ms = kv.second.total_ms;
        }
        n++;
    }
    ctx->stats.clear();
    return (int32_t)n;
}

}  // extern "C"
