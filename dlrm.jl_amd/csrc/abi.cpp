// abi.cpp — the extern "C" boundary declared in include/dlrm_hip.h.
//
// Owns the handle types (ctx, tables, indexer, the optimizers'), validates arguments on the host,
// maps HIP errors to dlrm_status codes and forwards to the kernel launchers.  No launching
// entry point allocates or synchronises (hipGraph-capturable).  An optimizer rule is described
// once, in kRules; the entry points bind it to their call (bind_rule) and pass that down.  Which index
// build a batch takes is decided once, in build_plan.hpp's plan_build; the entry points that build are
// checks -> plan -> begin_build -> the launch (run_build, or the forward / backward / apply launch that
// carries the build) -> record_build.
#include <dlfcn.h>
#include <execinfo.h>
#include <hip/hip_runtime.h>
#include <signal.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "common.hpp"
#include "apply.hpp"
#include "q8.hpp"

using namespace dlrm;

struct dlrm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // side stream + fork/join events: work that depends only on the indices (the hash indexer
    // build) runs beside the forward; graph capture follows the fork and the join
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    unsigned* err = nullptr;  // device error word
    // host-visible copy of it (pinned), refreshed by dlrm_error_snapshot on the stream and read by
    // dlrm_error_peek without touching the GPU: bounds errors of deferred work reach the host
    // without a per-step synchronisation
    volatile unsigned* err_host = nullptr;
    int cus = 256;
    char msg[512] = {0};
};

struct dlrm_tables {
    dlrm_ctx* ctx = nullptr;
    int T = 0, D = 0, dtype = 0;
    TableDesc* d_desc = nullptr;
    std::vector<TableDesc> h_desc;
    bool aligned16 = true;
};

// int8 row-quantized tables: the caller's code and {scale, bias} arrays
struct dlrm_q8_tables {
    dlrm_ctx* ctx = nullptr;
    int T = 0, D = 0;
    Q8Desc* d_desc = nullptr;
    std::vector<Q8Desc> h_desc;
    int64_t rows = 0;  // of every table
    int q_align = 16;  // the largest power of two <= 16 that divides every q pointer (q8_plan.hpp)
};

// An optimizer's state of one table set: the caller's per-table pointers, uploaded once
struct StateDims {
    int T = 0, D = 0;  // what the handle was created for
};
template <typename E>
struct StatePtrs : StateDims {
    bool aligned16 = true;  // every pointer is 16-B aligned
    E** d_ptr = nullptr;
    std::vector<E*> h_ptr;
};
// Sparse Adagrad: fp32 state
struct dlrm_adagrad : StatePtrs<float> {
    bool rowwise = false;  // one word per table row instead of one row
    // the stochastic kind (dlrm_adagrad_create_sr): bf16 tables, the weights' store rounded with the seed and the step
    bool stochastic = false;
    uint64_t seed = 0;
    uint64_t* d_step = nullptr;  // one device word, as dlrm_sr_sgd's
};
// The low halves of split-bf16 tables
struct dlrm_split_sgd : StatePtrs<uint16_t> {};
// Stochastically rounded SGD on bf16 tables: no per-row state, a seed and one device word, the step
struct dlrm_sr_sgd : StateDims {
    uint64_t seed = 0;
    uint64_t* d_step = nullptr;
};

// An optimizer rule on the host: what every call site asks of one, indexed by kRule* (common.hpp).  The arithmetic
// is the units' (apply.hpp, interact.hip); a rule bound to a call is a BoundRule.
struct RuleDesc {
    const char* update_fn;  // its entry points, for the messages: the update ...
    const char* step_fn;    // ... and the training step's backward (its _prepare form: the same with the suffix)
    const char* name;       // the rule in words
    const char* made;       // its handle in words ("... created for %d tables"); NULL: none
    const char* bf16_only;  // why its tables are bfloat16; NULL: fp32 too
    const char* no_atomic;  // why it has no atomic mode (an atomic add never holds a row's whole sum or step); NULL:
                            // it has one
    unsigned bit;           // of dlrm_indexer_state, when its step backward stepped a build's once-hit rows
    ApplyFn* apply;         // the update's apply launch
    ApplyFn* step_apply;    // the training step's
};
static const RuleDesc kRules[kNumRules] = {
    {"dlrm_sgd_update", "dlrm_step_bwd", "Descent", nullptr, nullptr, nullptr, 0u, launch_sgd_apply, launch_sgd_apply},
    {"dlrm_split_sgd_update", "dlrm_split_step_bwd", "the split rule", "the low halves were",
     "split tables are bf16 (the high halves)", "a row's two halves are stepped together", DLRM_IX_SINGLES_SPLIT,
     launch_split_sgd_apply, launch_split_step_apply},
    // (the two Adagrad rules share their entry points: the kind comes from the handle)
    {"dlrm_adagrad_update", "dlrm_adagrad_step_bwd", "the element-wise Adagrad rule", "the optimizer state was", nullptr,
     "the rule needs each row's complete sum", DLRM_IX_SINGLES_ADAGRAD, launch_adagrad_apply, launch_adagrad_step_apply},
    {"dlrm_adagrad_update", "dlrm_adagrad_step_bwd", "the row-wise Adagrad rule", "the optimizer state was", nullptr,
     "the rule needs each row's complete sum", DLRM_IX_SINGLES_ROWWISE, launch_rowwise_adagrad_apply,
     launch_rowwise_adagrad_step_apply},
    {"dlrm_sr_sgd_update", "dlrm_sr_step_bwd", "the stochastic rule", "the optimizer was",
     "stochastic rounding is of bf16 tables (fp32: nothing to round)", "the rule rounds each row's complete step once",
     DLRM_IX_SINGLES_STOCHASTIC, launch_sr_sgd_apply, launch_sr_step_apply},
    // (the Adagrad rules of a dlrm_adagrad_create_sr handle: a step backward of their own, dlrm_sr_adagrad_step_bwd --
    // dlrm_adagrad_step_bwd refuses the handle)
    {"dlrm_adagrad_update", "dlrm_sr_adagrad_step_bwd", "the stochastic element-wise Adagrad rule", "the optimizer state was",
     "stochastic rounding is of bf16 tables (fp32: nothing to round)", "the rule needs each row's complete sum",
     DLRM_IX_SINGLES_SR_ADAGRAD, launch_sr_adagrad_apply, launch_sr_adagrad_step_apply},
    {"dlrm_adagrad_update", "dlrm_sr_adagrad_step_bwd", "the stochastic row-wise Adagrad rule", "the optimizer state was",
     "stochastic rounding is of bf16 tables (fp32: nothing to round)", "the rule needs each row's complete sum",
     DLRM_IX_SINGLES_SR_ROWWISE, launch_sr_rowwise_adagrad_apply, launch_sr_rowwise_adagrad_step_apply},
};

// The rule of a call, from its handle and scalars
static BoundRule bind_rule(float lr) {
    BoundRule r;
    r.lr = lr;
    return r;
}
static BoundRule bind_rule(const dlrm_split_sgd* op, float lr) {
    BoundRule r = bind_rule(lr);
    r.kind = kRuleSplit;
    r.state = op->d_ptr;
    r.aligned16 = op->aligned16;
    r.handle = op;
    return r;
}
static BoundRule bind_rule(const dlrm_adagrad* op, float lr, float eps) {
    BoundRule r = bind_rule(lr);
    r.kind = op->stochastic ? (op->rowwise ? kRuleStochasticRowwise : kRuleStochasticAdagrad)
                            : (op->rowwise ? kRuleRowwise : kRuleAdagrad);
    r.seed = op->seed;
    r.step = op->d_step;
    r.eps = eps;
    r.state = op->d_ptr;
    r.aligned16 = op->rowwise || op->aligned16;  // (a row-wise state word is loaded alone)
    r.handle = op;
    return r;
}
static BoundRule bind_rule(const dlrm_sr_sgd* op, float lr) {
    BoundRule r = bind_rule(lr);
    r.kind = kRuleStochastic;
    r.seed = op->seed;
    r.step = op->d_step;
    r.handle = op;
    return r;
}

struct dlrm_indexer {
    dlrm_ctx* ctx = nullptr;
    int T = 0;
    int parts_log2 = 0;  // the wave builds of <= 2048 positions per table: log2 parts (0: the default, 16)
    int TV = 0;  // tables of the per-table arrays: 4T when the forward launch may split tables by row bits
    IndexerDev dev{};
    void* block = nullptr;  // one allocation for every array
    size_t bytes = 0;       // its size
    void* partial_big = nullptr;  // partial rows for D > kPartialDim (allocated on first use)
    // recorded by the last build
    bool built = false;
    bool split = false;  // built by dlrm_step_fwd's kernel: once-hit rows are left to the backward
    bool prepared = false;  // built by dlrm_step_bwd_prepare for the next dlrm_step_fwd (not yet consumed)
    bool singles_done = false;  // a split backward has applied this build's once-hit rows already
    int singles_rule = 0;  // ... with this rule (kRule*) ...
    const StateDims* singles_handle = nullptr;  // ... bound to this handle (check_completes)
    // device words for the bounds errors of builds that may run beside a step's write-deciding
    // kernels, which read the ctx's flag to decide whether to write (raising there would be a race,
    // ADVICE r5): [0] dlrm_indexer_prepare (a side-stream build beside the current step; cleared
    // before each build, folded into the ctx's flag by the apply of this indexer), [1] the NEXT
    // batch's build inside an apply launch (dlrm_step_bwd_prepare; nothing reads it).  Either way the
    // forward / lookup of the same indices raises their errors on the ctx's flag.
    unsigned* prep_err = nullptr;
    const void* indices = nullptr;
    int itype = 0, base = 0, B = 0, L = 0;
    int64_t tstride = 0;
};

namespace dlrm {
unsigned* ctx_error_word(dlrm_ctx* ctx) { return ctx->err; }
hipStream_t ctx_stream(dlrm_ctx* ctx) { return ctx->stream; }
int ctx_num_cus(dlrm_ctx* ctx) { return ctx->cus; }
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
const Knobs& knobs() {
    static const Knobs k{env_int("DLRM_STEP_PARTS", 0),       env_int("DLRM_BUILD_PARTS", 0),
                         env_int("DLRM_RELU_2PASS", 1) == 0, env_int("DLRM_BWD_YS", 1) == 0,
                         env_int("DLRM_BWD_SPLIT", 1) == 0,  env_int("DLRM_BWD_SPB", 0),
                         env_int("DLRM_BWD_CPL", 0),         env_int("DLRM_UPD_SBU", 1),
                         env_int("DLRM_WAVE_ROUNDS", 0),     env_int("DLRM_BAG_WAVE", 1) == 0,
                         env_int("DLRM_BAG_VS", 0),          env_int("DLRM_BAG_SPLIT", 1)};
    return k;
}
int ctx_device(dlrm_ctx* ctx) { return ctx->device; }
int ctx_fail(dlrm_ctx* ctx, int code, const char* fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->msg, sizeof(ctx->msg), fmt, ap);
        va_end(ap);
    }
    return code;
}
int ctx_hip(dlrm_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return DLRM_OK;
    return ctx_fail(ctx, e == hipErrorOutOfMemory ? DLRM_E_NOMEM : DLRM_E_HIP, "%s: %s", what, hipGetErrorString(e));
}
}  // namespace dlrm

#define CHECK_ARG(cond, ...) \
    do {                     \
        if (!(cond)) return ctx_fail(ctx, DLRM_E_ARG, __VA_ARGS__); \
    } while (0)

static int hip_set(dlrm_ctx* ctx) { return ctx_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"); }

// ---- an indexer's build: plan (build_plan.hpp plan_build) -> begin_build -> the launch -> record_build
static IndexerShape shape_of(const dlrm_indexer* ix) {
    return IndexerShape{ix->dev.cap, ix->T, ix->TV, ix->dev.hsize, ix->parts_log2};
}

// The index arguments a build was made from, remembered for built_from
struct IndexArgs {
    const void* indices;
    int itype;
    int64_t tstride;
    int base, B, L;
};

// The word a build raises its bounds errors on
static unsigned* err_word(dlrm_ctx* ctx, const dlrm_indexer* ix, ErrWord w) {
    return w == ErrWord::Ctx ? ctx->err : ix->prep_err + (w == ErrWord::Prep1 ? 1 : 0);
}

// The only place that changes an indexer's record before a launch: whatever it held is gone (Kept: a prepared
// build is consumed by the forward that gathers with it, and stands)
static void begin_build(dlrm_indexer* ix, const BuildPlan& p) {
    ix->prepared = false;
    if (p.form == BuildForm::Kept) return;
    ix->built = false;
    ix->dev.vshift = p.vshift;
}

// ... and the only one that writes it after a launch that went out
static void record_build(dlrm_indexer* ix, const BuildPlan& p, const IndexArgs& a) {
    ix->built = true;
    ix->split = p.split;
    ix->prepared = p.prepared;
    ix->singles_done = false;
    ix->singles_rule = kRuleDescent;
    ix->singles_handle = nullptr;
    ix->dev.has_map = p.has_map ? 1 : 0;
    ix->dev.build_err = p.build_err ? err_word(ix->ctx, ix, p.err) : nullptr;
    ix->indices = a.indices;
    ix->itype = a.itype;
    ix->tstride = a.tstride;
    ix->base = a.base;
    ix->B = a.B;
    ix->L = a.L;
}

static bool built_from(const dlrm_indexer* ix, const void* indices, int itype, int64_t tstride, int base, int B,
                       int L) {
    return ix->built && ix->indices == indices && ix->B == B && ix->L == L && ix->itype == itype &&
           ix->tstride == tstride && ix->base == base;
}

static int ensure_side(dlrm_ctx* ctx) {
    if (ctx->side) return DLRM_OK;
    int rc = ctx_hip(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking), "hipStreamCreate(side)");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming), "hipEventCreate");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming), "hipEventCreate");
    return rc;
}

// The words of a create's messages: "FN: null WHAT", "FN: table %d has no ONE", "hipMalloc(HIP)".
struct StateWords { const char *fn, *what, *one, *hip; };

// The checks of a state handle's create, the upload of its per-table pointers and the unwinding.
// (Rows of D elements from a 16-B aligned base are aligned when the row's bytes % 16 == 0, which the vector
// kernels need anyway.)
template <typename OP, typename E>
static int state_create(dlrm_ctx* ctx, const dlrm_tables* tb, bool bf16_only, E* const* ptrs, OP** out,
                        const StateWords& w) {
    CHECK_ARG(ctx && tb && out, "%s: null argument", w.fn);
    *out = nullptr;
    CHECK_ARG(!bf16_only || tb->dtype == DLRM_BF16, "%s: split tables are bf16 (the high halves)", w.fn);
    CHECK_ARG(tb->T == 0 || ptrs, "%s: null %s", w.fn, w.what);
    for (int t = 0; t < tb->T; ++t)
        CHECK_ARG(ptrs[t] || tb->h_desc[t].nrows == 0, "%s: table %d has no %s", w.fn, t, w.one);
    OP* op = new (std::nothrow) OP();
    if (!op) return DLRM_E_NOMEM;
    op->T = tb->T;
    op->D = tb->D;
    op->h_ptr.assign(ptrs, ptrs + tb->T);
    for (int t = 0; t < tb->T; ++t)
        if ((uintptr_t)ptrs[t] % 16) op->aligned16 = false;
    char what[2][48];
    snprintf(what[0], sizeof(what[0]), "hipMalloc(%s)", w.hip);
    snprintf(what[1], sizeof(what[1]), "hipMemcpy(%s)", w.hip);
    int rc = hip_set(ctx);
    if (rc == DLRM_OK && tb->T > 0) {
        rc = ctx_hip(ctx, hipMalloc((void**)&op->d_ptr, sizeof(E*) * tb->T), what[0]);
        if (rc == DLRM_OK)
            rc = ctx_hip(ctx, hipMemcpy(op->d_ptr, op->h_ptr.data(), sizeof(E*) * tb->T, hipMemcpyHostToDevice), what[1]);
    }
    if (rc != DLRM_OK) {
        if (op->d_ptr) (void)hipFree(op->d_ptr);
        delete op;
        return rc;
    }
    *out = op;
    return DLRM_OK;
}

template <typename OP>
static int state_destroy(OP* op) {
    if (!op) return DLRM_OK;
    if (op->d_ptr) (void)hipFree(op->d_ptr);
    delete op;
    return DLRM_OK;
}

extern "C" {

int dlrm_abi_version(void) { return DLRM_HIP_ABI_VERSION; }

int dlrm_ctx_create(int device, void* stream, dlrm_ctx** out) {
    if (!out) return DLRM_E_ARG;
    *out = nullptr;
    dlrm_ctx* ctx = new (std::nothrow) dlrm_ctx();
    if (!ctx) return DLRM_E_NOMEM;
    ctx->device = device;
    ctx->stream = (hipStream_t)stream;
    int rc = hip_set(ctx);
    if (rc == DLRM_OK) {
        hipDeviceProp_t prop;
        rc = ctx_hip(ctx, hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
        if (rc == DLRM_OK) ctx->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMalloc((void**)&ctx->err, 16), "hipMalloc(err)");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMemset(ctx->err, 0, 16), "hipMemset(err)");
    if (rc == DLRM_OK) {
        void* h = nullptr;
        rc = ctx_hip(ctx, hipHostMalloc(&h, 64, hipHostMallocMapped), "hipHostMalloc(err_host)");
        if (rc == DLRM_OK) {
            memset(h, 0, 64);
            ctx->err_host = (volatile unsigned*)h;
            void* dh = nullptr;  // its device address, kept in the error word's second half
            rc = ctx_hip(ctx, hipHostGetDevicePointer(&dh, h, 0), "hipHostGetDevicePointer(err_host)");
            if (rc == DLRM_OK)
                rc = ctx_hip(ctx, hipMemcpy((char*)ctx->err + 8, &dh, sizeof(dh), hipMemcpyHostToDevice),
                             "write err_host address");
        }
    }
    if (rc != DLRM_OK) {
        if (ctx->err) (void)hipFree(ctx->err);
        if (ctx->err_host) (void)hipHostFree((void*)ctx->err_host);
        delete ctx;
        return rc;
    }
    *out = ctx;
    return DLRM_OK;
}

int dlrm_ctx_destroy(dlrm_ctx* ctx) {
    if (!ctx) return DLRM_OK;
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    if (ctx->err) (void)hipFree(ctx->err);
    if (ctx->err_host) (void)hipHostFree((void*)ctx->err_host);
    delete ctx;
    return DLRM_OK;
}

int dlrm_ctx_set_stream(dlrm_ctx* ctx, void* stream) {
    if (!ctx) return DLRM_E_ARG;
    ctx->stream = (hipStream_t)stream;
    return DLRM_OK;
}

const char* dlrm_last_error(const dlrm_ctx* ctx) { return ctx ? ctx->msg : "null context"; }

int dlrm_sync(dlrm_ctx* ctx) {
    if (!ctx) return DLRM_E_ARG;
    return ctx_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

int dlrm_check_bounds(dlrm_ctx* ctx) {
    if (!ctx) return DLRM_E_ARG;
    unsigned h = 0;
    int rc = ctx_hip(ctx, hipMemcpyAsync(&h, ctx->err, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream),
                     "read error word");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMemsetAsync(ctx->err, 0, sizeof(unsigned), ctx->stream), "clear error word");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (rc != DLRM_OK) return rc;
    ctx->err_host[0] = 0;  // (the flag is clear now; a stale snapshot must not report it again)
    if (h & kErrIndex) return ctx_fail(ctx, DLRM_E_INDEX, "BoundsError: an embedding index was out of range");
    return DLRM_OK;
}

int dlrm_error_snapshot(dlrm_ctx* ctx) {
    if (!ctx) return DLRM_E_ARG;
    return ctx_hip(ctx, hipMemcpyAsync((void*)ctx->err_host, ctx->err, sizeof(unsigned), hipMemcpyDeviceToHost,
                                       ctx->stream),
                   "dlrm_error_snapshot");
}

int dlrm_error_peek(const dlrm_ctx* ctx, unsigned* word) {
    if (!ctx || !word) return DLRM_E_ARG;
    *word = ctx->err_host[0];
    return DLRM_OK;
}

int dlrm_malloc(dlrm_ctx* ctx, size_t bytes, void** dptr) {
    CHECK_ARG(ctx && dptr, "dlrm_malloc: null argument");
    *dptr = nullptr;
    if (bytes == 0) return DLRM_OK;
    return ctx_hip(ctx, hipMalloc(dptr, bytes), "hipMalloc");
}

int dlrm_free(dlrm_ctx* ctx, void* dptr) {
    CHECK_ARG(ctx, "dlrm_free: null ctx");
    if (!dptr) return DLRM_OK;
    return ctx_hip(ctx, hipFree(dptr), "hipFree");
}

int dlrm_memcpy_h2d(dlrm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    CHECK_ARG(ctx && (bytes == 0 || (dst && src)), "dlrm_memcpy_h2d: null argument");
    int rc = ctx_hip(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "memcpy h2d");
    return rc ? rc : ctx_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

int dlrm_memcpy_h2d_async(dlrm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    CHECK_ARG(ctx && (bytes == 0 || (dst && src)), "dlrm_memcpy_h2d_async: null argument");
    return ctx_hip(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "memcpy h2d async");
}

int dlrm_host_register(void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return DLRM_E_ARG;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? DLRM_OK : DLRM_E_HIP;
}

int dlrm_host_unregister(void* ptr) {
    if (!ptr) return DLRM_E_ARG;
    return hipHostUnregister(ptr) == hipSuccess ? DLRM_OK : DLRM_E_HIP;
}

int dlrm_memcpy_d2h(dlrm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    CHECK_ARG(ctx && (bytes == 0 || (dst && src)), "dlrm_memcpy_d2h: null argument");
    int rc = ctx_hip(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream), "memcpy d2h");
    return rc ? rc : ctx_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

// ---------------------------------------------------------------------------- tables
int dlrm_tables_create(dlrm_ctx* ctx, int num_tables, int dim, int dtype, void* const* data, const int64_t* nrows,
                       dlrm_tables** out) {
    CHECK_ARG(ctx && out, "dlrm_tables_create: null argument");
    *out = nullptr;
    CHECK_ARG(num_tables >= 0 && dim > 0, "dlrm_tables_create: num_tables=%d dim=%d", num_tables, dim);
    CHECK_ARG(dtype == DLRM_F32 || dtype == DLRM_BF16, "dlrm_tables_create: unknown dtype %d", dtype);
    CHECK_ARG(num_tables == 0 || (data && nrows), "dlrm_tables_create: null data/nrows");
    dlrm_tables* tb = new (std::nothrow) dlrm_tables();
    if (!tb) return DLRM_E_NOMEM;
    tb->ctx = ctx;
    tb->T = num_tables;
    tb->D = dim;
    tb->dtype = dtype;
    tb->h_desc.resize(num_tables);
    for (int t = 0; t < num_tables; ++t) {
        if (nrows[t] < 0 || nrows[t] >= 0xFFFFFFFFll || (nrows[t] > 0 && !data[t])) {
            delete tb;
            return ctx_fail(ctx, DLRM_E_ARG, "dlrm_tables_create: table %d has nrows=%lld", t, (long long)nrows[t]);
        }
        tb->h_desc[t].data = data[t];
        tb->h_desc[t].nrows = nrows[t];
        if ((uintptr_t)data[t] % 16) tb->aligned16 = false;
    }
    int rc = hip_set(ctx);
    if (rc == DLRM_OK && num_tables > 0) {
        rc = ctx_hip(ctx, hipMalloc((void**)&tb->d_desc, sizeof(TableDesc) * num_tables), "hipMalloc(tables)");
        if (rc == DLRM_OK)
            rc = ctx_hip(ctx, hipMemcpy(tb->d_desc, tb->h_desc.data(), sizeof(TableDesc) * num_tables,
                                        hipMemcpyHostToDevice), "hipMemcpy(tables)");
    }
    if (rc != DLRM_OK) {
        if (tb->d_desc) (void)hipFree(tb->d_desc);
        delete tb;
        return rc;
    }
    *out = tb;
    return DLRM_OK;
}

int dlrm_tables_destroy(dlrm_tables* tb) {
    if (!tb) return DLRM_OK;
    if (tb->d_desc) (void)hipFree(tb->d_desc);
    delete tb;
    return DLRM_OK;
}

static int check_indices(dlrm_ctx* ctx, const dlrm_tables* tb, const void* indices, int itype, int64_t tstride,
                         int batch, int lookups) {
    CHECK_ARG(itype == DLRM_I32 || itype == DLRM_I64, "unknown index type %d", itype);
    CHECK_ARG(batch >= 0 && lookups >= 1, "batch=%d lookups=%d", batch, lookups);
    CHECK_ARG((int64_t)batch * lookups < (1ll << 31), "batch*lookups exceeds 2^31");
    CHECK_ARG(batch == 0 || tb->T == 0 || indices, "null indices");
    CHECK_ARG(tb->T <= 1 || tstride >= (int64_t)batch * lookups, "table_stride %lld < batch*lookups %lld",
              (long long)tstride, (long long)batch * lookups);
    return DLRM_OK;
}

int dlrm_maplookup(dlrm_ctx* ctx, const dlrm_tables* tb, const void* indices, int itype, int64_t table_stride,
                   int index_base, int batch, int lookups, void* out, int64_t out_ld, int64_t out_offset) {
    CHECK_ARG(ctx && tb, "dlrm_maplookup: null ctx/tables");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, lookups);
    if (rc) return rc;
    CHECK_ARG(batch == 0 || tb->T == 0 || out, "dlrm_maplookup: null out");
    CHECK_ARG(out_offset >= 0 && out_ld >= out_offset + (int64_t)tb->T * tb->D,
              "dlrm_maplookup: out_ld %lld < out_offset %lld + T*D %lld", (long long)out_ld, (long long)out_offset,
              (long long)tb->T * tb->D);
    return launch_maplookup(ctx, tb->d_desc, tb->aligned16, tb->T, tb->D, tb->dtype, indices, itype, table_stride,
                            index_base, batch, lookups, out, out_ld, out_offset, tb->h_desc.data());
}

int dlrm_maplookup_blocked(dlrm_ctx* ctx, const dlrm_tables* tb, const void* indices, int itype,
                           int64_t table_stride, int index_base, int batch, int lookups, void* out, int64_t out_ld,
                           int64_t out_offset, int64_t out_table_stride, int64_t block_rows, int64_t block_stride) {
    CHECK_ARG(ctx && tb, "dlrm_maplookup_blocked: null ctx/tables");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, lookups);
    if (rc) return rc;
    CHECK_ARG(batch == 0 || tb->T == 0 || out, "dlrm_maplookup_blocked: null out");
    CHECK_ARG(out_ld >= 0 && out_offset >= 0 && out_table_stride >= 0 && block_rows > 0 && block_stride >= 0,
              "dlrm_maplookup_blocked: negative stride or block_rows < 1");
    return launch_maplookup_map(ctx, tb->d_desc, tb->aligned16, tb->T, tb->D, tb->dtype, indices, itype,
                                table_stride, index_base, batch, lookups, out,
                                OutMap{out_ld, out_offset, out_table_stride, block_rows, block_stride},
                                tb->h_desc.data());
}

int dlrm_scatter_rows(dlrm_ctx* ctx, int esize, int num_tables, int batch, int dim, const void* src, int64_t src_ld,
                      int64_t src_offset, void* dst, const int64_t* dst_base, const int64_t* dst_ld) {
    CHECK_ARG(ctx, "dlrm_scatter_rows: null ctx");
    CHECK_ARG(esize == 2 || esize == 4, "dlrm_scatter_rows: esize %d", esize);
    CHECK_ARG(num_tables >= 0 && batch >= 0 && dim >= 0 && src_ld >= 0 && src_offset >= 0,
              "dlrm_scatter_rows: negative size");
    CHECK_ARG(num_tables == 0 || batch == 0 || dim == 0 || (src && dst && dst_base && dst_ld),
              "dlrm_scatter_rows: null buffer");
    // 16-B pieces when the source rows allow (a destination row that is not 16-B aligned is
    // copied element by element on the device)
    const int u = 16 / esize;
    const bool vec = (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0 && src_ld % u == 0 && src_offset % u == 0 &&
                     dim % u == 0;
    return launch_scatter_rows(ctx, esize, num_tables, batch, dim, src, src_ld, src_offset, dst, dst_base, dst_ld,
                               vec);
}

// ---------------------------------------------------------------------- dense seams
int dlrm_bce_head(dlrm_ctx* ctx, int batch, const float* logits, int64_t logits_ld, const float* labels, float* prob,
                  float* dlogit, float* loss, float* dbias) {
    CHECK_ARG(ctx, "dlrm_bce_head: null ctx");
    CHECK_ARG(batch >= 1 && logits_ld >= 1, "dlrm_bce_head: batch=%d logits_ld=%lld", batch, (long long)logits_ld);
    CHECK_ARG(logits && labels && prob && dlogit && loss, "dlrm_bce_head: null buffer");
    return launch_bce_head(ctx, batch, logits, logits_ld, labels, prob, dlogit, loss, dbias);
}

// ---------------------------------------------------------------------- evaluation
int dlrm_eval_layout(int* bins, int* shift, int64_t* words) {
    if (!bins || !shift || !words) return DLRM_E_ARG;
    *bins = kEvalBins;
    *shift = kEvalShift;
    *words = kEvalWords;
    return DLRM_OK;
}

int dlrm_eval_accumulate(dlrm_ctx* ctx, int64_t* state, int batch, const float* scores, int64_t scores_ld, int is_prob,
                         const float* labels, float* prob) {
    CHECK_ARG(ctx, "dlrm_eval_accumulate: null ctx");
    CHECK_ARG(batch >= 1 && scores_ld >= 1, "dlrm_eval_accumulate: batch=%d scores_ld=%lld", batch,
              (long long)scores_ld);
    CHECK_ARG(state && scores && labels, "dlrm_eval_accumulate: null buffer");
    CHECK_ARG((uintptr_t)state % 8 == 0, "dlrm_eval_accumulate: state must be 8-B aligned");
    return launch_eval_accumulate(ctx, reinterpret_cast<unsigned long long*>(state), batch, scores, scores_ld,
                                  is_prob != 0, labels, prob);
}

int dlrm_relu_bwd_bias_workspace(int batch, int n, int64_t* work_floats, int64_t* counters) {
    if (batch < 0 || n < 0 || !work_floats || !counters) return DLRM_E_ARG;
    *work_floats = relu_bwd_chunks(batch) * (int64_t)n;
    *counters = relu_bwd_groups(n);
    return DLRM_OK;
}

int dlrm_relu_bwd_bias(dlrm_ctx* ctx, int batch, int n, const float* y, int64_t y_ld, float* g, int64_t g_ld,
                       float* dbias, float* work, unsigned* counters) {
    CHECK_ARG(ctx, "dlrm_relu_bwd_bias: null ctx");
    CHECK_ARG(batch >= 0 && n >= 0 && n % 4 == 0, "dlrm_relu_bwd_bias: batch=%d n=%d (n %% 4 == 0)", batch, n);
    CHECK_ARG(y_ld >= n && g_ld >= n && y_ld % 4 == 0 && g_ld % 4 == 0, "dlrm_relu_bwd_bias: leading dimensions");
    if (batch == 0 || n == 0) return DLRM_OK;
    CHECK_ARG(y && g && dbias && work && counters, "dlrm_relu_bwd_bias: null buffer");
    CHECK_ARG((uintptr_t)y % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)dbias % 16 == 0 &&
                  (uintptr_t)work % 16 == 0,
              "dlrm_relu_bwd_bias: buffers must be 16-B aligned");
    return launch_relu_bwd_bias(ctx, batch, n, y, y_ld, g, g_ld, dbias, work, counters);
}

int dlrm_dac_decode(dlrm_ctx* ctx, const dlrm_dac_record* records, int batch, float* labels, float* dense,
                    int64_t dense_ld, void* sparse, int itype, int64_t table_stride) {
    CHECK_ARG(ctx, "dlrm_dac_decode: null ctx");
    CHECK_ARG(batch >= 0 && dense_ld >= 13 && table_stride >= batch, "dlrm_dac_decode: batch=%d dense_ld=%lld "
              "table_stride=%lld", batch, (long long)dense_ld, (long long)table_stride);
    CHECK_ARG(itype == DLRM_I32 || itype == DLRM_I64, "dlrm_dac_decode: itype %d", itype);
    CHECK_ARG(batch == 0 || (records && labels && dense && sparse), "dlrm_dac_decode: null buffer");
    CHECK_ARG((uintptr_t)records % 4 == 0, "dlrm_dac_decode: records must be 4-B aligned");
    return launch_dac_decode(ctx, records, batch, labels, dense, dense_ld, sparse, itype, table_stride);
}

// ---------------------------------------------------------------------- interaction
int dlrm_interact_fwd(dlrm_ctx* ctx, int dtype, int d, int num_features, int batch, const void* x, int64_t x_ld,
                      void* ys, int64_t ys_ld, void* out, int64_t out_ld, int padding) {
    CHECK_ARG(ctx, "dlrm_interact_fwd: null ctx");
    CHECK_ARG(dtype == DLRM_F32 || dtype == DLRM_BF16, "dlrm_interact_fwd: dtype %d", dtype);
    CHECK_ARG(d > 0 && num_features >= 1 && batch >= 0 && padding >= 0, "dlrm_interact_fwd: d=%d F=%d B=%d pad=%d", d,
              num_features, batch, padding);
    const int64_t P = (int64_t)num_features * (num_features - 1) / 2;
    CHECK_ARG(x_ld >= d && ys_ld >= (int64_t)num_features * d && out_ld >= d + P + padding,
              "dlrm_interact_fwd: leading dimensions too small");
    CHECK_ARG(batch == 0 || (x && ys && out), "dlrm_interact_fwd: null buffer");
    return launch_interact_fwd(ctx, dtype, d, num_features, batch, x, x_ld, ys, ys_ld, out, out_ld, padding);
}

int dlrm_lookup_interact_fwd(dlrm_ctx* ctx, const dlrm_tables* tb, const void* indices, int itype,
                             int64_t table_stride, int index_base, int batch, int lookups, const void* x,
                             int64_t x_ld, void* ys, int64_t ys_ld, void* out, int64_t out_ld, int padding) {
    CHECK_ARG(ctx && tb, "dlrm_lookup_interact_fwd: null ctx/tables");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, lookups);
    if (rc) return rc;
    const int d = tb->D, F = tb->T + 1;
    const int64_t P = (int64_t)F * (F - 1) / 2;
    CHECK_ARG(padding >= 0 && x_ld >= d && (!ys || ys_ld >= (int64_t)F * d) && out_ld >= d + P + padding,
              "dlrm_lookup_interact_fwd: leading dimensions too small");
    CHECK_ARG(batch == 0 || (x && out), "dlrm_lookup_interact_fwd: null buffer");
    rc = launch_lookup_interact_fwd(ctx, tb->d_desc, tb->aligned16, tb->T, tb->dtype, indices, itype, table_stride,
                                    index_base, lookups, d, batch, x, x_ld, ys, ys_ld, out, out_ld, padding, tb->h_desc.data());
    if (rc != DLRM_E_UNSUPPORTED) return rc;
    if (!ys)
        return ctx_fail(ctx, DLRM_E_UNSUPPORTED,
                        "dlrm_lookup_interact_fwd: ys may be NULL only where the fused kernel applies "
                        "(16-B aligned rows, F <= 96)");
    rc = launch_maplookup(ctx, tb->d_desc, tb->aligned16, tb->T, tb->D, tb->dtype, indices, itype, table_stride,
                          index_base, batch, lookups, ys, ys_ld, d, tb->h_desc.data());
    if (rc) return rc;
    return launch_interact_fwd(ctx, tb->dtype, d, F, batch, x, x_ld, ys, ys_ld, out, out_ld, padding);
}

// ------------------------------------------------------------- int8 row-quantized tables
int dlrm_q8_tables_create(dlrm_ctx* ctx, int num_tables, int dim, uint8_t* const* q, float* const* sb,
                          const int64_t* nrows, dlrm_q8_tables** out) {
    CHECK_ARG(ctx && out, "dlrm_q8_tables_create: null argument");
    *out = nullptr;
    CHECK_ARG(num_tables >= 0 && dim > 0, "dlrm_q8_tables_create: num_tables=%d dim=%d", num_tables, dim);
    CHECK_ARG(num_tables == 0 || (q && sb && nrows), "dlrm_q8_tables_create: null q/sb/nrows");
    for (int t = 0; t < num_tables; ++t) {
        CHECK_ARG(nrows[t] >= 0 && nrows[t] < 0xFFFFFFFFll && (nrows[t] == 0 || (q[t] && sb[t])),
                  "dlrm_q8_tables_create: table %d has nrows=%lld", t, (long long)nrows[t]);
        CHECK_ARG((uintptr_t)sb[t] % 8 == 0, "dlrm_q8_tables_create: sb[%d] is not 8-B aligned", t);
    }
    dlrm_q8_tables* qt = new (std::nothrow) dlrm_q8_tables();
    if (!qt) return DLRM_E_NOMEM;
    qt->ctx = ctx;
    qt->T = num_tables;
    qt->D = dim;
    qt->h_desc.resize(num_tables);
    for (int t = 0; t < num_tables; ++t) {
        qt->h_desc[t] = Q8Desc{q[t], (float2*)sb[t], nrows[t], qt->rows};
        qt->rows += nrows[t];
        while (qt->q_align > 1 && (uintptr_t)q[t] % (unsigned)qt->q_align) qt->q_align >>= 1;
    }
    int rc = hip_set(ctx);
    if (rc == DLRM_OK && num_tables > 0) {
        rc = ctx_hip(ctx, hipMalloc((void**)&qt->d_desc, sizeof(Q8Desc) * num_tables), "hipMalloc(q8 tables)");
        if (rc == DLRM_OK)
            rc = ctx_hip(ctx, hipMemcpy(qt->d_desc, qt->h_desc.data(), sizeof(Q8Desc) * num_tables, hipMemcpyHostToDevice),
                         "hipMemcpy(q8 tables)");
    }
    if (rc != DLRM_OK) {
        if (qt->d_desc) (void)hipFree(qt->d_desc);
        delete qt;
        return rc;
    }
    *out = qt;
    return DLRM_OK;
}

int dlrm_q8_tables_destroy(dlrm_q8_tables* q8) {
    if (!q8) return DLRM_OK;
    if (q8->d_desc) (void)hipFree(q8->d_desc);
    delete q8;
    return DLRM_OK;
}

// the two sets describe the same rows
static int check_q8_pair(dlrm_ctx* ctx, const dlrm_tables* tb, const dlrm_q8_tables* q8, const char* fn) {
    CHECK_ARG(tb->T == q8->T && tb->D == q8->D, "%s: %d tables of dim %d against %d quantized tables of dim %d", fn, tb->T,
              tb->D, q8->T, q8->D);
    for (int t = 0; t < tb->T; ++t)
        CHECK_ARG(tb->h_desc[t].nrows == q8->h_desc[t].nrows, "%s: table %d has %lld rows against %lld quantized rows", fn,
                  t, (long long)tb->h_desc[t].nrows, (long long)q8->h_desc[t].nrows);
    return DLRM_OK;
}

int dlrm_q8_quantize(dlrm_ctx* ctx, const dlrm_tables* src, dlrm_q8_tables* dst) {
    CHECK_ARG(ctx && src && dst, "dlrm_q8_quantize: null ctx/tables");
    const int rc = check_q8_pair(ctx, src, dst, "dlrm_q8_quantize");
    if (rc) return rc;
    return launch_q8_quantize(ctx, src->d_desc, src->dtype, src->aligned16, dst->d_desc, dst->q_align, dst->T, dst->D,
                              dst->rows);
}

int dlrm_q8_dequantize(dlrm_ctx* ctx, const dlrm_q8_tables* src, dlrm_tables* dst) {
    CHECK_ARG(ctx && src && dst, "dlrm_q8_dequantize: null ctx/tables");
    const int rc = check_q8_pair(ctx, dst, src, "dlrm_q8_dequantize");
    if (rc) return rc;
    return launch_q8_dequantize(ctx, src->d_desc, src->q_align, dst->d_desc, dst->dtype, dst->aligned16, src->T, src->D,
                                src->rows);
}

static int check_q8_indices(dlrm_ctx* ctx, const dlrm_q8_tables* q8, const void* indices, int itype, int64_t tstride,
                            int batch, int lookups, int dtype) {
    CHECK_ARG(dtype == DLRM_F32 || dtype == DLRM_BF16, "unknown dtype %d", dtype);
    CHECK_ARG(itype == DLRM_I32 || itype == DLRM_I64, "unknown index type %d", itype);
    CHECK_ARG(batch >= 0 && lookups >= 1, "batch=%d lookups=%d", batch, lookups);
    CHECK_ARG((int64_t)batch * lookups < (1ll << 31), "batch*lookups exceeds 2^31");
    CHECK_ARG(batch == 0 || q8->T == 0 || indices, "null indices");
    CHECK_ARG(q8->T <= 1 || tstride >= (int64_t)batch * lookups, "table_stride %lld < batch*lookups %lld",
              (long long)tstride, (long long)batch * lookups);
    return DLRM_OK;
}

int dlrm_q8_maplookup(dlrm_ctx* ctx, const dlrm_q8_tables* q8, const void* indices, int itype, int64_t table_stride,
                      int index_base, int batch, int lookups, int dtype, void* out, int64_t out_ld, int64_t out_offset) {
    CHECK_ARG(ctx && q8, "dlrm_q8_maplookup: null ctx/tables");
    const int rc = check_q8_indices(ctx, q8, indices, itype, table_stride, batch, lookups, dtype);
    if (rc) return rc;
    CHECK_ARG(batch == 0 || q8->T == 0 || out, "dlrm_q8_maplookup: null out");
    CHECK_ARG(out_offset >= 0 && out_ld >= out_offset + (int64_t)q8->T * q8->D,
              "dlrm_q8_maplookup: out_ld %lld < out_offset %lld + T*D %lld", (long long)out_ld, (long long)out_offset,
              (long long)q8->T * q8->D);
    return launch_q8_maplookup(ctx, q8->d_desc, q8->q_align, q8->T, q8->D, indices, itype, table_stride, index_base,
                               batch, lookups, dtype, out, out_ld, out_offset);
}

int dlrm_q8_lookup_interact_fwd(dlrm_ctx* ctx, const dlrm_q8_tables* q8, const void* indices, int itype,
                                int64_t table_stride, int index_base, int batch, int lookups, int dtype, const void* x,
                                int64_t x_ld, void* out, int64_t out_ld, int padding) {
    CHECK_ARG(ctx && q8, "dlrm_q8_lookup_interact_fwd: null ctx/tables");
    const int rc = check_q8_indices(ctx, q8, indices, itype, table_stride, batch, lookups, dtype);
    if (rc) return rc;
    const int d = q8->D, F = q8->T + 1;
    const int64_t P = (int64_t)F * (F - 1) / 2;
    CHECK_ARG(padding >= 0 && x_ld >= d && out_ld >= d + P + padding,
              "dlrm_q8_lookup_interact_fwd: leading dimensions too small");
    CHECK_ARG(batch == 0 || (x && out), "dlrm_q8_lookup_interact_fwd: null buffer");
    return launch_q8_lookup_interact_fwd(ctx, q8->h_desc.data(), q8->q_align, q8->T, d, indices, itype, table_stride,
                                         index_base, batch, lookups, dtype, x, x_ld, out, out_ld, padding);
}

int dlrm_interact_bwd(dlrm_ctx* ctx, int dtype, int d, int num_features, int batch, const void* dout, int64_t dout_ld,
                      int padding, const void* t, int64_t t_ld, float* dx, int64_t dx_ld, float* dt, int64_t dt_ld) {
    CHECK_ARG(ctx, "dlrm_interact_bwd: null ctx");
    CHECK_ARG(dtype == DLRM_F32 || dtype == DLRM_BF16, "dlrm_interact_bwd: dtype %d", dtype);
    CHECK_ARG(d > 0 && num_features >= 1 && batch >= 0 && padding >= 0, "dlrm_interact_bwd: d=%d F=%d B=%d", d,
              num_features, batch);
    const int64_t P = (int64_t)num_features * (num_features - 1) / 2;
    CHECK_ARG(dout_ld >= d + P + padding && t_ld >= (int64_t)num_features * d && dx_ld >= d &&
                  dt_ld >= (int64_t)num_features * d,
              "dlrm_interact_bwd: leading dimensions too small");
    CHECK_ARG(batch == 0 || (dout && t && dx && dt), "dlrm_interact_bwd: null buffer");
    return launch_interact_bwd(ctx, dtype, d, num_features, batch, dout, dout_ld, t, t_ld, dx, dx_ld, dt, dt_ld);
}

// ---- Implementation 2 pieces (interact.jl:176-215, :503-551)
int dlrm_triangular_slice(dlrm_ctx* ctx, int dtype, int sz, int batch, const void* z, int64_t z_batch_stride,
                          void* out, int64_t out_ld) {
    CHECK_ARG(ctx, "dlrm_triangular_slice: null ctx");
    CHECK_ARG(dtype == DLRM_F32 || dtype == DLRM_BF16, "dlrm_triangular_slice: dtype %d", dtype);
    CHECK_ARG(sz >= 1 && batch >= 0, "dlrm_triangular_slice: sz=%d batch=%d", sz, batch);
    CHECK_ARG(z_batch_stride >= (int64_t)sz * sz && out_ld >= (int64_t)sz * (sz - 1) / 2,
              "dlrm_triangular_slice: strides too small");
    CHECK_ARG(batch == 0 || sz < 2 || (z && out), "dlrm_triangular_slice: null buffer");  // sz = 1: no pairs
    return launch_triangular_slice(ctx, dtype, sz, batch, z, z_batch_stride, out, out_ld);
}

int dlrm_triangular_slice_back(dlrm_ctx* ctx, int dtype, int sz, int batch, const void* dy, int64_t dy_ld, void* a,
                               int64_t a_batch_stride, int symmetric) {
    CHECK_ARG(ctx, "dlrm_triangular_slice_back: null ctx");
    CHECK_ARG(dtype == DLRM_F32 || dtype == DLRM_BF16, "dlrm_triangular_slice_back: dtype %d", dtype);
    CHECK_ARG(sz >= 1 && batch >= 0, "dlrm_triangular_slice_back: sz=%d batch=%d", sz, batch);
    CHECK_ARG(a_batch_stride >= (int64_t)sz * sz && dy_ld >= (int64_t)sz * (sz - 1) / 2,
              "dlrm_triangular_slice_back: strides too small");
    CHECK_ARG(batch == 0 || (a && (sz < 2 || dy)), "dlrm_triangular_slice_back: null buffer");
    return launch_triangular_slice_back(ctx, dtype, sz, batch, dy, dy_ld, a, a_batch_stride, symmetric ? 1 : 0);
}

int dlrm_self_batched_mul(dlrm_ctx* ctx, int dtype, int d, int num_features, int batch, const void* t, int64_t t_ld,
                          void* z, int64_t z_batch_stride) {
    CHECK_ARG(ctx, "dlrm_self_batched_mul: null ctx");
    CHECK_ARG(dtype == DLRM_F32 || dtype == DLRM_BF16, "dlrm_self_batched_mul: dtype %d", dtype);
    CHECK_ARG(d > 0 && num_features >= 1 && batch >= 0, "dlrm_self_batched_mul: d=%d F=%d B=%d", d, num_features, batch);
    if (num_features > 90) return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "dlrm_self_batched_mul: F=%d > 90", num_features);
    CHECK_ARG(t_ld >= (int64_t)num_features * d && z_batch_stride >= (int64_t)num_features * num_features,
              "dlrm_self_batched_mul: strides too small");
    CHECK_ARG(batch == 0 || (t && z), "dlrm_self_batched_mul: null buffer");
    return launch_self_batched_mul(ctx, dtype, d, num_features, batch, t, t_ld, z, z_batch_stride);
}

int dlrm_self_batched_mul_back(dlrm_ctx* ctx, int dtype, int d, int num_features, int batch, const void* t,
                               int64_t t_ld, const void* dz, int64_t dz_batch_stride, float* dt, int64_t dt_ld) {
    CHECK_ARG(ctx, "dlrm_self_batched_mul_back: null ctx");
    CHECK_ARG(dtype == DLRM_F32 || dtype == DLRM_BF16, "dlrm_self_batched_mul_back: dtype %d", dtype);
    CHECK_ARG(d > 0 && num_features >= 1 && batch >= 0, "dlrm_self_batched_mul_back: d=%d F=%d B=%d", d, num_features,
              batch);
    if (num_features > 90)
        return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "dlrm_self_batched_mul_back: F=%d > 90", num_features);
    CHECK_ARG(t_ld >= (int64_t)num_features * d && dz_batch_stride >= (int64_t)num_features * num_features &&
                  dt_ld >= (int64_t)num_features * d,
              "dlrm_self_batched_mul_back: strides too small");
    CHECK_ARG(batch == 0 || (t && dz && dt), "dlrm_self_batched_mul_back: null buffer");
    return launch_self_batched_mul_back(ctx, dtype, d, num_features, batch, t, t_ld, dz, dz_batch_stride, dt, dt_ld);
}

int dlrm_interact_bwd_gather(dlrm_ctx* ctx, const dlrm_tables* tb, dlrm_indexer* ix, const void* indices, int itype,
                             int64_t table_stride, int index_base, int batch, int lookups, const void* x,
                             int64_t x_ld, const void* dout, int64_t dout_ld, int padding, float* dx, int64_t dx_ld,
                             float* dt, int64_t dt_ld) {
    CHECK_ARG(ctx && tb, "dlrm_interact_bwd_gather: null ctx/tables");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, lookups);
    if (rc) return rc;
    CHECK_ARG(lookups == 1, "dlrm_interact_bwd_gather: one-hot lookups only (L=%d: use dlrm_interact_bwd on ys)",
              lookups);
    const int d = tb->D, F = tb->T + 1;
    const int64_t P = (int64_t)F * (F - 1) / 2;
    CHECK_ARG(padding >= 0 && x_ld >= d && dout_ld >= d + P + padding && dx_ld >= d && dt_ld >= (int64_t)F * d,
              "dlrm_interact_bwd_gather: leading dimensions too small");
    CHECK_ARG(batch == 0 || (x && dout && dx && dt), "dlrm_interact_bwd_gather: null buffer");
    if (ix) {
        CHECK_ARG(tb->T == ix->T, "dlrm_interact_bwd_gather: indexer has %d tables, tables has %d", ix->T, tb->T);
        CHECK_ARG((int64_t)batch * lookups <= ix->dev.cap,
                  "dlrm_interact_bwd_gather: batch*lookups %lld > indexer capacity %lld", (long long)batch * lookups,
                  (long long)ix->dev.cap);
    }
    const BuildPlan plan = plan_build(BuildSite::BwdGather, IndexerShape{}, batch, knobs(), BuildCaps{});
    if (ix) begin_build(ix, plan);
    rc = launch_interact_bwd_gather(ctx, tb->d_desc, tb->aligned16, tb->T, tb->dtype, indices, itype, table_stride,
                                    index_base, lookups, d, batch, x, x_ld, dout, dout_ld, dx, dx_ld, dt, dt_ld,
                                    ix ? &ix->dev : nullptr);
    if (rc || !ix) return rc;
    // as dlrm_indexer_build: a following update may pass DLRM_UPDATE_PREBUILT
    record_build(ix, plan, IndexArgs{indices, itype, table_stride, index_base, batch, lookups});
    return DLRM_OK;
}

int dlrm_interact_bwd_blocked(dlrm_ctx* ctx, const dlrm_tables* tb, const void* indices, int itype,
                              int64_t table_stride, int index_base, int batch, const void* x, int64_t x_ld,
                              const void* dout, int64_t dout_ld, int padding, float* dx, int64_t dx_ld, float* dst,
                              const int64_t* dst_base, const int64_t* dst_ld) {
    CHECK_ARG(ctx && tb, "dlrm_interact_bwd_blocked: null ctx/tables");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, 1);
    if (rc) return rc;
    const int d = tb->D, F = tb->T + 1;
    const int64_t P = (int64_t)F * (F - 1) / 2;
    CHECK_ARG(padding >= 0 && x_ld >= d && dout_ld >= d + P + padding && dx_ld >= d,
              "dlrm_interact_bwd_blocked: leading dimensions too small");
    CHECK_ARG(batch == 0 || tb->T == 0 || (x && dout && dx && dst && dst_base && dst_ld),
              "dlrm_interact_bwd_blocked: null buffer");
    return launch_interact_bwd_blocked(ctx, tb->d_desc, tb->aligned16, tb->T, tb->dtype, indices, itype, table_stride,
                                       index_base, 1, d, batch, x, x_ld, dout, dout_ld, dx, dx_ld, dst, dst_base,
                                       dst_ld);
}

// --------------------------------------------------------------------------- indexer
// Footprint.  The per-part arrays (perm, seg_start, seg_row, chunks, hot, hot_slice, hot_cnt: 92 B
// per slot; + 20 B of HBM sort scratch above 2048 positions) are cap slots per table: the wave
// builds pack a table's parts back to back (common.hpp kSegPad, "compact" layout), whatever the
// parts (256 per table at 32768 positions).  Only the in-LDS parts build of 4096 < N <= 8192
// (fast_index_table, 8 parts, v * cap) needs 8 virtual tables of cap slots per table, so an
// indexer whose cap is in that range is carved with 8.  (Round 5 gave every wave-build part a whole
// cap and re-carved on first use: 128 x the table at 16384 positions, ~7 GB per indexer for 26
// tables)  Partial rows of multi-slice hot segments are per real table (the wave
// build's item map indexes them by its flat slice number, at most pcap per table), times the <= 8
// parts of the builds without an item map.
static int64_t partial_rows(const dlrm_indexer* ix) {
    const int64_t T0 = ix->T > 0 ? ix->T : 1;
    const int64_t cap = ix->dev.cap;
    const int np = cap <= kPartsMaxN ? 8 : 1;
    return T0 * np * ix->dev.pcap;
}

// Carves every array of the indexer for `parts` virtual tables per table (contents reset).
static int indexer_carve(dlrm_ctx* ctx, dlrm_indexer* ix, int parts) {
    const int64_t cap = ix->dev.cap;
    const int64_t T0 = ix->T > 0 ? ix->T : 1;
    const int64_t T = (int64_t)parts * T0;
    const int64_t hs = ix->dev.hsize;
    // the largest wave build this indexer takes: 2^vw parts per table, T0 << vw / 4 workgroups (>= 64
    // parts: the builds of <= 2048 positions may take 32 or 64, dlrm_indexer_set_parts)
    const int vw = std::max(wave_vshift(cap < kWaveMaxN ? cap : kWaveMaxN), 6);
    const int64_t TW = T0 << vw;
    // carve every array out of one allocation (16-B aligned pieces)
    struct Piece { void** p; size_t bytes; };
    const size_t n = (size_t)(T * cap), n0 = (size_t)(T0 * cap);
    const size_t n1 = (size_t)std::max(T * (cap + 1), T0 * (cap + kSegPad));  // (compact: a sentinel per part)
    const size_t ncnt = (size_t)std::max(T, TW);
    // the wave build's flat item lists: kResLists sub-lists of res_stride records (indexer.hpp); the
    // HBM sort scratch (5 arrays, compact) for the builds of more than 2048 positions
    const size_t nrec = (size_t)kResLists * (size_t)res_stride((int)(TW / 4), cap, vw) + 64;
    const int64_t wstride = cap > kStepIndexMaxN ? T0 * cap + 64 : 0;
    IndexerDev d = ix->dev;
    float* partial_keep = ix->partial_big ? d.partial : nullptr;  // (a grown partial buffer stays)
    Piece pieces[] = {
        {(void**)&d.keys0, n0 * 4},    {(void**)&d.keys1, n0 * 4},  {(void**)&d.vals0, n0 * 4},
        {(void**)&d.vals1, n0 * 4},    {(void**)&d.perm, n * 4},    {(void**)&d.seg_start, n1 * 4},
        {(void**)&d.seg_row, n * 4},   {(void**)&d.chunks, n * 32}, {(void**)&d.hot, n * 16},
        {(void**)&d.hot_slice, n * 16}, {(void**)&d.hot_cnt, n * 4},
        {(void**)&d.partial, partial_keep ? 0 : (size_t)partial_rows(ix) * kPartialDim * 4},
        {(void**)&d.counts, ncnt * 32},   {(void**)&d.single, n0},
        {(void**)&ix->prep_err, 16},
        {(void**)&d.slice_rec, nrec * 32}, {(void**)&d.chunk_rec, nrec * 32},
        {(void**)&d.wscratch, (size_t)wstride * 5 * 4},
        {(void**)&d.item_tot, 64},     {(void**)&d.build_arrive, 2048},
        // hash indexer arrays (only when a build can exceed the in-LDS indexer's kFastMaxN)
        {(void**)&d.pslot, hs ? n0 * 4 : 0},   {(void**)&d.hent, (size_t)(T0 * hs) * 8},
        {(void**)&d.hseg, (size_t)(T0 * hs) * 8},
        {(void**)&d.hfill, (size_t)(T0 * hs) * 4}, {(void**)&d.hstate, hs ? (size_t)T0 * 32 : 0},
    };
    size_t total = 0;
    for (auto& pc : pieces) total += (pc.bytes + 255) & ~(size_t)255;
    int rc = hip_set(ctx);
    void* block = nullptr;
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMalloc(&block, total), "hipMalloc(indexer)");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMemset(block, 0, total), "hipMemset(indexer)");
    char* base = (char*)block;
    if (rc == DLRM_OK)
        for (auto& pc : pieces) {
            *pc.p = pc.bytes ? base : nullptr;
            base += (pc.bytes + 255) & ~(size_t)255;
        }
    if (rc == DLRM_OK && hs)  // every slot starts empty (the alloc pass resets the slots it used)
        rc = ctx_hip(ctx, hipMemset(d.hent, 0xff, (size_t)(T0 * hs) * 8), "hipMemset(hash slots)");
    if (rc != DLRM_OK) {
        if (block) (void)hipFree(block);
        return rc;
    }
    if (partial_keep) d.partial = partial_keep;
    d.wstride = wstride;
    if (ix->block) {  // (nothing in flight may still read the old arrays)
        (void)hipDeviceSynchronize();
        (void)hipFree(ix->block);
    }
    ix->block = block;
    ix->dev = d;
    ix->TV = (int)T;
    ix->bytes = total;
    ix->built = ix->prepared = ix->singles_done = false;
    ix->singles_rule = kRuleDescent;
    ix->singles_handle = nullptr;
    ix->dev.has_map = 0;
    ix->dev.build_err = nullptr;
    return DLRM_OK;
}

int dlrm_indexer_create(dlrm_ctx* ctx, int num_tables, int64_t max_lookups, dlrm_indexer** out) {
    CHECK_ARG(ctx && out, "dlrm_indexer_create: null argument");
    *out = nullptr;
    CHECK_ARG(num_tables >= 0 && max_lookups >= 0 && max_lookups < (1ll << 31), "dlrm_indexer_create: T=%d cap=%lld",
              num_tables, (long long)max_lookups);
    dlrm_indexer* ix = new (std::nothrow) dlrm_indexer();
    if (!ix) return DLRM_E_NOMEM;
    ix->ctx = ctx;
    ix->T = num_tables;
    const int64_t cap = max_lookups > 0 ? max_lookups : 1;
    ix->dev.cap = cap;
    ix->dev.pcap = indexer_slice_cap(cap);
    ix->dev.pdim = kPartialDim;
    ix->dev.chunk_max = kChunk;
    const int64_t hs = carve_hash(cap) ? hix_table_slots(cap) : 0;
    ix->dev.hsize = hs;
    ix->dev.hbits = 0;
    while (((int64_t)1 << ix->dev.hbits) < hs) ++ix->dev.hbits;
    const int rc = indexer_carve(ctx, ix, carve_virtual_tables(cap));
    if (rc != DLRM_OK) {
        delete ix;
        return rc;
    }
    *out = ix;
    return DLRM_OK;
}

int dlrm_indexer_set_chunk(dlrm_ctx* ctx, dlrm_indexer* ix, int max_positions) {
    CHECK_ARG(ctx && ix, "dlrm_indexer_set_chunk: null argument");
    CHECK_ARG(max_positions == 16 || max_positions == 32, "dlrm_indexer_set_chunk: %d (16 or 32)", max_positions);
    ix->dev.chunk_max = max_positions;
    return DLRM_OK;
}

int dlrm_indexer_set_parts(dlrm_ctx* ctx, dlrm_indexer* ix, int parts) {
    CHECK_ARG(ctx && ix, "dlrm_indexer_set_parts: null argument");
    CHECK_ARG(parts == 0 || parts == 16 || parts == 32 || parts == 64, "dlrm_indexer_set_parts: %d (0, 16, 32 or 64)",
              parts);
    ix->parts_log2 = parts == 64 ? 6 : (parts == 32 ? 5 : (parts == 16 ? 4 : 0));
    return DLRM_OK;
}

int dlrm_indexer_reserve(dlrm_ctx* ctx, dlrm_indexer* ix, int batch) {
    CHECK_ARG(ctx && ix, "dlrm_indexer_reserve: null argument");
    CHECK_ARG(batch >= 0 && batch <= ix->dev.cap, "dlrm_indexer_reserve: batch %d > capacity %lld", batch,
              (long long)ix->dev.cap);
    // (round 6: the wave builds' compact layout needs no re-carving; nothing to do)
    return DLRM_OK;
}

int dlrm_indexer_bytes(const dlrm_indexer* ix, int64_t* bytes) {
    if (!ix || !bytes) return DLRM_E_ARG;
    *bytes = (int64_t)ix->bytes + (ix->partial_big ? partial_rows(ix) * (int64_t)ix->dev.pdim * 4 : 0);
    return DLRM_OK;
}

int dlrm_indexer_destroy(dlrm_indexer* ix) {
    if (!ix) return DLRM_OK;
    if (ix->block) (void)hipFree(ix->block);
    if (ix->partial_big) (void)hipFree(ix->partial_big);
    delete ix;
    return DLRM_OK;
}

// The entry point's words for a plan that refuses (BuildForm::None with DLRM_E_UNSUPPORTED)
static int refuse_build(dlrm_ctx* ctx, BuildSite site, int64_t N) {
    if (site == BuildSite::Prepare)
        return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "dlrm_indexer_prepare: batch %d (the wave build: batch <= %d, "
                        "tables x capacity < 2^31)", (int)N, kWaveMaxN);
    return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "split indexer build: %lld positions per table", (long long)N);
}

// The launch of a build that has one of its own, by the plan's form (after begin_build)
static int run_build(dlrm_ctx* ctx, dlrm_indexer* ix, const dlrm_tables* tb, const BuildPlan& p, const IndexArgs& a) {
    const int64_t N = (int64_t)a.B * a.L;
    unsigned* const err = err_word(ctx, ix, p.err);
    // (an indexer's own word starts each build clear: the apply of this indexer folds it into the ctx's flag)
    if (p.err == ErrWord::Prep0) {
        const int rc = ctx_hip(ctx, hipMemsetAsync(err, 0, sizeof(unsigned), ctx->stream), "clear build bounds word");
        if (rc) return rc;
    }
    switch (p.form) {
    case BuildForm::Bag:
        return launch_bag_build(ctx, ix->dev, tb->d_desc, tb->T, a.indices, a.itype, a.tstride, a.base, (int)N, err);
    case BuildForm::Wave:
        return launch_step_prepare(ctx, ix->dev, tb->d_desc, tb->T, a.indices, a.itype, a.tstride, a.base, (int)N, err);
    default:  // Lds2, Lds4, LdsParts, Hash, Sorted (the builds inside another launch are their entry point's)
        return launch_indexer_build(ctx, ix->dev, tb->d_desc, tb->T, a.indices, a.itype, a.tstride, a.base, a.B, a.L,
                                    p.form, p.split, err, p.side ? ctx->side : nullptr);
    }
}

// plan -> begin -> launch -> record, for the sites whose build is a launch of its own
static int build_now(dlrm_ctx* ctx, dlrm_indexer* ix, const dlrm_tables* tb, BuildSite site, const IndexArgs& a,
                     const BuildCaps& caps) {
    const int64_t N = (int64_t)a.B * a.L;
    const BuildPlan p = plan_build(site, shape_of(ix), N, knobs(), caps);
    if (p.form == BuildForm::None) return refuse_build(ctx, site, N);  // (a refused call leaves the indexer as it was)
    begin_build(ix, p);
    const int rc = run_build(ctx, ix, tb, p, a);
    if (rc) return rc;
    record_build(ix, p, a);
    return DLRM_OK;
}

int dlrm_indexer_build(dlrm_ctx* ctx, dlrm_indexer* ix, const dlrm_tables* tb, const void* indices, int itype,
                       int64_t table_stride, int index_base, int batch, int lookups) {
    CHECK_ARG(ctx && ix && tb, "dlrm_indexer_build: null argument");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, lookups);
    if (rc) return rc;
    CHECK_ARG(tb->T == ix->T, "dlrm_indexer_build: indexer has %d tables, tables has %d", ix->T, tb->T);
    CHECK_ARG((int64_t)batch * lookups <= ix->dev.cap, "dlrm_indexer_build: batch*lookups %lld > capacity %lld",
              (long long)batch * lookups, (long long)ix->dev.cap);
    return build_now(ctx, ix, tb, BuildSite::Build, IndexArgs{indices, itype, table_stride, index_base, batch, lookups},
                     BuildCaps{});
}

int dlrm_indexer_build_split(dlrm_ctx* ctx, dlrm_indexer* ix, const dlrm_tables* tb, const void* indices, int itype,
                             int64_t table_stride, int index_base, int batch) {
    CHECK_ARG(ctx && ix && tb, "dlrm_indexer_build_split: null argument");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, 1);
    if (rc) return rc;
    CHECK_ARG(tb->T == ix->T, "dlrm_indexer_build_split: indexer has %d tables, tables has %d", ix->T, tb->T);
    CHECK_ARG(batch <= ix->dev.cap, "dlrm_indexer_build_split: batch %d > capacity %lld", batch,
              (long long)ix->dev.cap);
    return build_now(ctx, ix, tb, BuildSite::BuildSplit, IndexArgs{indices, itype, table_stride, index_base, batch, 1},
                     BuildCaps{});
}

int dlrm_indexer_prepare(dlrm_ctx* ctx, dlrm_indexer* ix, const dlrm_tables* tb, const void* indices, int itype,
                         int64_t table_stride, int index_base, int batch) {
    CHECK_ARG(ctx && ix && tb, "dlrm_indexer_prepare: null argument");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, 1);
    if (rc) return rc;
    CHECK_ARG(tb->T == ix->T, "dlrm_indexer_prepare: indexer has %d tables, tables has %d", ix->T, tb->T);
    CHECK_ARG(batch <= ix->dev.cap, "dlrm_indexer_prepare: batch %d > capacity %lld", batch, (long long)ix->dev.cap);
    // bounds errors go to the indexer's own word, not the ctx's flag (the plan's ErrWord::Prep0): this build usually
    // runs on a side stream beside the current step, whose kernels read the ctx's flag to decide whether to write
    // their rows.  The next forward / lookup of these indices raises them on the ctx's flag; the apply of this
    // indexer folds the word in as well (a prebuilt update without a lookup).
    BuildCaps caps{};
    caps.idx_vec32 = idx_vec32(indices, itype, table_stride);
    caps.cus = ctx->cus;
    return build_now(ctx, ix, tb, BuildSite::Prepare, IndexArgs{indices, itype, table_stride, index_base, batch, 1}, caps);
}

// One (virtual) table's build, whole: rows, grouped positions, segment starts.
struct IndexerTable {
    std::vector<uint32_t> rows;
    std::vector<int32_t> perm, seg_start;
};
static int read_indexer_table(dlrm_ctx* ctx, const dlrm_indexer* ix, int v, IndexerTable& o) {
    int32_t cnt[8];
    int rc = ctx_hip(ctx, hipMemcpy(cnt, ix->dev.counts + (int64_t)v * 8, sizeof(cnt), hipMemcpyDeviceToHost), "read");
    if (rc) return rc;
    const int64_t U = cnt[0], NV = cnt[4];
    // (a wave build's parts are packed per table: IndexerDev::part_off / seg_off)
    const int vs = ix->dev.vshift;
    const int64_t cap = ix->dev.cap;
    const int64_t off = ix->dev.has_map ? (int64_t)(v >> vs) * cap + cnt[kCntOff] : (int64_t)v * cap;
    const int64_t soff = ix->dev.has_map ? (int64_t)(v >> vs) * (cap + kSegPad) + cnt[kCntOff] + (v & ((1 << vs) - 1))
                                         : (int64_t)v * (cap + 1);
    o.rows.resize(U);
    o.perm.resize(NV);
    o.seg_start.resize(U + 1);
    if (U) rc = ctx_hip(ctx, hipMemcpy(o.rows.data(), ix->dev.seg_row + off, U * 4, hipMemcpyDeviceToHost), "read");
    if (rc == DLRM_OK && NV)
        rc = ctx_hip(ctx, hipMemcpy(o.perm.data(), ix->dev.perm + off, NV * 4, hipMemcpyDeviceToHost), "read");
    if (rc == DLRM_OK)
        rc = ctx_hip(ctx, hipMemcpy(o.seg_start.data(), ix->dev.seg_start + soff,
                                    (U + 1) * 4, hipMemcpyDeviceToHost), "read");
    return rc;
}

int dlrm_indexer_state(const dlrm_indexer* ix, unsigned* state) {
    if (!ix || !state) return DLRM_E_ARG;
    *state = (ix->built ? DLRM_IX_BUILT : 0u) | (ix->split ? DLRM_IX_SPLIT : 0u) |
             (ix->prepared ? DLRM_IX_PREPARED : 0u) | (ix->singles_done ? DLRM_IX_SINGLES_DONE : 0u) |
             (ix->singles_done ? kRules[ix->singles_rule].bit : 0u);
    return DLRM_OK;
}

int dlrm_indexer_read(dlrm_ctx* ctx, const dlrm_indexer* ix, int table, int64_t* num_unique, int64_t* rows,
                      int64_t* positions, int64_t* seg_start, int64_t cap) {
    CHECK_ARG(ctx && ix && num_unique, "dlrm_indexer_read: null argument");
    CHECK_ARG(ix->built, "dlrm_indexer_read: indexer not built");
    CHECK_ARG(table >= 0 && table < ix->T, "dlrm_indexer_read: table %d", table);
    int rc = ctx_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (rc) return rc;
    IndexerTable tt;
    if (ix->dev.vshift == 0) {
        rc = read_indexer_table(ctx, ix, table, tt);
    } else {
        // a forward-launch build: merge the table's parts (each sorted by row)
        const int np = 1 << ix->dev.vshift;
        std::vector<IndexerTable> h(np);
        for (int q = 0; q < np && rc == DLRM_OK; ++q) rc = read_indexer_table(ctx, ix, table * np + q, h[q]);
        std::vector<size_t> k(np, 0);
        tt.seg_start.assign(1, 0);
        for (;;) {
            int e = -1;
            for (int q = 0; q < np && rc == DLRM_OK; ++q)
                if (k[q] < h[q].rows.size() && (e < 0 || h[q].rows[k[q]] < h[e].rows[k[e]])) e = q;
            if (e < 0) break;
            const size_t u = k[e]++;
            tt.rows.push_back(h[e].rows[u]);
            for (int32_t i = h[e].seg_start[u]; i < h[e].seg_start[u + 1]; ++i) tt.perm.push_back(h[e].perm[i]);
            tt.seg_start.push_back((int32_t)tt.perm.size());
        }
    }
    if (rc) return rc;
    const int64_t U = (int64_t)tt.rows.size(), NV = (int64_t)tt.perm.size();
    *num_unique = U;
    if (rows)
        for (int64_t i = 0; i < U && i < cap; ++i) rows[i] = tt.rows[i];
    if (positions && seg_start) {
        for (int64_t i = 0; i < NV && i < cap; ++i) positions[i] = tt.perm[i];
        for (int64_t i = 0; i <= U && i <= cap; ++i) seg_start[i] = tt.seg_start[i];
    }
    return DLRM_OK;
}

// multi-slice hot segments keep partial rows of D elements (allocated on first use for D > kPartialDim;
// not on a launch path that is captured: the first update of a shape runs before capture)
static int ensure_partials(dlrm_ctx* ctx, dlrm_indexer* ix, int D) {
    if (D <= ix->dev.pdim) return DLRM_OK;
    void* p = nullptr;
    int rc = hip_set(ctx);
    if (rc == DLRM_OK)
        rc = ctx_hip(ctx, hipMalloc(&p, (size_t)partial_rows(ix) * D * 4), "hipMalloc(indexer partials)");
    if (rc) return rc;
    if (ix->partial_big) (void)hipFree(ix->partial_big);
    ix->partial_big = p;
    ix->dev.partial = (float*)p;
    ix->dev.pdim = D;
    return DLRM_OK;
}

// The rule's handle against the tables (the argument errors of the rule's update and of its training step)
static int check_rule(dlrm_ctx* ctx, const dlrm_tables* tb, const BoundRule& r, const char* fn) {
    const RuleDesc& d = kRules[r.kind];
    CHECK_ARG(!d.bf16_only || tb->dtype == DLRM_BF16, "%s: %s", fn, d.bf16_only);
    CHECK_ARG(!r.handle || (r.handle->T == tb->T && r.handle->D == tb->D), "%s: %s created for %d tables of dim %d", fn,
              d.made, r.handle ? r.handle->T : 0, r.handle ? r.handle->D : 0);
    return DLRM_OK;
}

// Who may complete whose backward.  A split backward stepped the build's once-hit rows with its rule and left their dt
// rows unwritten: only the same rule finishes what it started (dlrm_*_update(PREBUILT) and dlrm_*step_bwd(APPLY_ONLY)
// alike) -- another rule's rows hold another step -- and for the stochastic rule and the seeded Adagrad rules only the
// same handle: another one has another seed or step (and, Adagrad, another state).
static int check_completes(dlrm_ctx* ctx, const dlrm_indexer* ix, const BoundRule& r, const char* fn, const char* mode) {
    if (!ix->singles_done) return DLRM_OK;
    const bool same_rule = ix->singles_rule == r.kind;
    const bool seeded = r.kind == kRuleStochastic || r.kind == kRuleStochasticAdagrad || r.kind == kRuleStochasticRowwise;
    if (same_rule && (!seeded || ix->singles_handle == r.handle)) return DLRM_OK;
    const RuleDesc& by = kRules[ix->singles_rule];
    return ctx_fail(ctx, DLRM_E_STATE, "%s%s: a split backward (%s) already stepped this build's once-hit rows with %s%s",
                    fn, mode, by.step_fn, by.name, same_rule ? " of another handle" : "");
}

// The update entry points, from the index checks to the rule's launch.
static int rule_update(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_indexer* ix, const BoundRule& r, unsigned flags,
                       const void* indices, int itype, int64_t table_stride, int index_base, int batch, int lookups,
                       const void* grad, int grad_dtype, int64_t grad_ld, int64_t grad_offset) {
    const RuleDesc& d = kRules[r.kind];
    const char* const fn = d.update_fn;
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, lookups);
    if (rc == DLRM_OK) rc = check_rule(ctx, tb, r, fn);
    if (rc) return rc;
    CHECK_ARG(grad_dtype == DLRM_F32 || grad_dtype == DLRM_BF16, "%s: grad dtype %d", fn, grad_dtype);
    CHECK_ARG(grad_offset >= 0 && grad_ld >= grad_offset + (int64_t)tb->T * tb->D, "%s: grad_ld too small", fn);
    CHECK_ARG(batch == 0 || tb->T == 0 || grad, "%s: null grad", fn);
    if (flags & DLRM_UPDATE_ATOMIC) {  // (nothing is built)
        if (d.no_atomic) return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "%s: no atomic mode (%s)", fn, d.no_atomic);
        if (tb->dtype != DLRM_F32) return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "%s: atomic mode needs fp32 tables", fn);
        return launch_sgd_atomic(ctx, tb->d_desc, tb->T, tb->D, indices, itype, table_stride, index_base, batch,
                                 lookups, grad, grad_dtype, grad_ld, grad_offset, r.lr);  // (Descent: no other has the mode)
    }
    CHECK_ARG(ix, "%s: deterministic mode needs an indexer", fn);
    if (flags & DLRM_UPDATE_PREBUILT) {
        if (!built_from(ix, indices, itype, table_stride, index_base, batch, lookups))
            return ctx_fail(ctx, DLRM_E_STATE, "%s: indexer was not built from these indices", fn);
        rc = check_completes(ctx, ix, r, fn, "");
    } else {
        rc = dlrm_indexer_build(ctx, ix, tb, indices, itype, table_stride, index_base, batch, lookups);
    }
    if (rc == DLRM_OK) rc = ensure_partials(ctx, ix, tb->D);
    if (rc) return rc;
    // a split indexer (dlrm_indexer_build's default form, or dlrm_step_fwd's): its once-hit
    // positions are this launch's too -- unless a split backward (dlrm_step_bwd) has updated them
    // already, in which case only the repeated rows are left
    const SinglesArgs sa{(ix->split && !ix->singles_done) ? ix->dev.single : nullptr, indices, itype, table_stride,
                         index_base, batch * lookups};
    return d.apply(ctx, ix->dev, tb->d_desc, tb->aligned16 && r.aligned16, tb->T, tb->D, tb->dtype, lookups,
                   (int64_t)batch * lookups, grad, grad_dtype, grad_ld, grad_offset, r, sa, nullptr);
}

int dlrm_sgd_update(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_indexer* ix, unsigned flags, const void* indices, int itype,
                    int64_t table_stride, int index_base, int batch, int lookups, const void* grad, int grad_dtype,
                    int64_t grad_ld, int64_t grad_offset, float lr) {
    CHECK_ARG(ctx && tb, "dlrm_sgd_update: null ctx/tables");
    return rule_update(ctx, tb, ix, bind_rule(lr), flags, indices, itype, table_stride, index_base, batch, lookups, grad,
                       grad_dtype, grad_ld, grad_offset);
}

// ------------------------------------------------- optimizers with state: sparse Adagrad, split-bf16 tables
int dlrm_adagrad_create(dlrm_ctx* ctx, const dlrm_tables* tb, int rowwise, float* const* state, dlrm_adagrad** out) {
    const int rc = state_create(ctx, tb, false, state, out, {"dlrm_adagrad_create", "state", "state", "adagrad state"});
    if (rc == DLRM_OK) (*out)->rowwise = rowwise != 0;
    return rc;
}

int dlrm_adagrad_create_sr(dlrm_ctx* ctx, const dlrm_tables* tb, int rowwise, float* const* state, int64_t seed,
                           dlrm_adagrad** out) {
    CHECK_ARG(ctx && tb && out, "dlrm_adagrad_create_sr: null argument");
    *out = nullptr;
    CHECK_ARG(tb->dtype == DLRM_BF16, "dlrm_adagrad_create_sr: stochastic rounding is of bf16 tables (fp32: nothing to round)");
    // the Philox counter holds the table in 16 bits and the column's block of four in 16 bits
    CHECK_ARG(tb->T <= 65536 && (tb->D + 3) / 4 <= 65536, "dlrm_adagrad_create_sr: %d tables of dim %d (at most 65536 "
              "tables, dim / 4 at most 65536)", tb->T, tb->D);
    dlrm_adagrad* op = nullptr;
    int rc = state_create(ctx, tb, false, state, &op, {"dlrm_adagrad_create_sr", "state", "state", "adagrad state"});
    if (rc) return rc;
    op->rowwise = rowwise != 0;
    op->stochastic = true;
    op->seed = (uint64_t)seed;
    rc = ctx_hip(ctx, hipMalloc((void**)&op->d_step, sizeof(uint64_t)), "hipMalloc(adagrad step)");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMemset(op->d_step, 0, sizeof(uint64_t)), "hipMemset(adagrad step)");
    if (rc != DLRM_OK) {
        (void)dlrm_adagrad_destroy(op);
        return rc;
    }
    *out = op;
    return DLRM_OK;
}

int dlrm_adagrad_destroy(dlrm_adagrad* op) {
    if (op && op->d_step) (void)hipFree(op->d_step);
    return state_destroy(op);
}

int dlrm_adagrad_seek(dlrm_ctx* ctx, dlrm_adagrad* op, int64_t step) {
    CHECK_ARG(ctx && op, "dlrm_adagrad_seek: null ctx/optimizer");
    CHECK_ARG(op->stochastic, "dlrm_adagrad_seek: the handle has no step (dlrm_adagrad_create_sr makes one that has)");
    const int rc = hip_set(ctx);
    if (rc) return rc;
    return launch_sr_step_set(ctx, op->d_step, (uint64_t)step);
}

int dlrm_adagrad_step(dlrm_ctx* ctx, dlrm_adagrad* op, uint64_t* out) {
    CHECK_ARG(ctx && op && out, "dlrm_adagrad_step: null ctx/optimizer/out");
    CHECK_ARG(op->stochastic, "dlrm_adagrad_step: the handle has no step (dlrm_adagrad_create_sr makes one that has)");
    int rc = hip_set(ctx);
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (rc == DLRM_OK)
        rc = ctx_hip(ctx, hipMemcpy(out, op->d_step, sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(adagrad step)");
    return rc;
}

int dlrm_adagrad_update(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_adagrad* op, dlrm_indexer* ix, unsigned flags,
                        const void* indices, int itype, int64_t table_stride, int index_base, int batch, int lookups,
                        const void* grad, int grad_dtype, int64_t grad_ld, int64_t grad_offset, float lr, float eps) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_adagrad_update: null ctx/tables/optimizer/indexer");
    return rule_update(ctx, tb, ix, bind_rule(op, lr, eps), flags, indices, itype, table_stride, index_base, batch, lookups,
                       grad, grad_dtype, grad_ld, grad_offset);
}

int dlrm_split_sgd_create(dlrm_ctx* ctx, const dlrm_tables* tb, uint16_t* const* lo, dlrm_split_sgd** out) {
    return state_create(ctx, tb, true, lo, out, {"dlrm_split_sgd_create", "low halves", "low half", "split low halves"});
}

int dlrm_split_sgd_destroy(dlrm_split_sgd* op) { return state_destroy(op); }

int dlrm_split_sgd_update(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_split_sgd* op, dlrm_indexer* ix, unsigned flags,
                          const void* indices, int itype, int64_t table_stride, int index_base, int batch, int lookups,
                          const void* grad, int grad_dtype, int64_t grad_ld, int64_t grad_offset, float lr) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_split_sgd_update: null ctx/tables/optimizer/indexer");
    return rule_update(ctx, tb, ix, bind_rule(op, lr), flags, indices, itype, table_stride, index_base, batch, lookups, grad,
                       grad_dtype, grad_ld, grad_offset);
}

int dlrm_sr_sgd_create(dlrm_ctx* ctx, const dlrm_tables* tb, int64_t seed, dlrm_sr_sgd** out) {
    CHECK_ARG(ctx && tb && out, "dlrm_sr_sgd_create: null argument");
    *out = nullptr;
    CHECK_ARG(tb->dtype == DLRM_BF16, "dlrm_sr_sgd_create: stochastic rounding is of bf16 tables (fp32: nothing to round)");
    // the Philox counter holds the table in 16 bits and the column's block of four in 16 bits
    CHECK_ARG(tb->T <= 65536 && (tb->D + 3) / 4 <= 65536, "dlrm_sr_sgd_create: %d tables of dim %d (at most 65536 tables, "
              "dim / 4 at most 65536)", tb->T, tb->D);
    dlrm_sr_sgd* op = new (std::nothrow) dlrm_sr_sgd();
    if (!op) return DLRM_E_NOMEM;
    op->T = tb->T;
    op->D = tb->D;
    op->seed = (uint64_t)seed;
    int rc = hip_set(ctx);
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMalloc((void**)&op->d_step, sizeof(uint64_t)), "hipMalloc(sr step)");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMemset(op->d_step, 0, sizeof(uint64_t)), "hipMemset(sr step)");
    if (rc != DLRM_OK) {
        if (op->d_step) (void)hipFree(op->d_step);
        delete op;
        return rc;
    }
    *out = op;
    return DLRM_OK;
}

int dlrm_sr_sgd_destroy(dlrm_sr_sgd* op) {
    if (!op) return DLRM_OK;
    if (op->d_step) (void)hipFree(op->d_step);
    delete op;
    return DLRM_OK;
}

int dlrm_sr_sgd_update(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_sr_sgd* op, dlrm_indexer* ix, unsigned flags,
                       const void* indices, int itype, int64_t table_stride, int index_base, int batch, int lookups,
                       const void* grad, int grad_dtype, int64_t grad_ld, int64_t grad_offset, float lr) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_sr_sgd_update: null ctx/tables/optimizer/indexer");
    return rule_update(ctx, tb, ix, bind_rule(op, lr), flags, indices, itype, table_stride, index_base, batch, lookups, grad,
                       grad_dtype, grad_ld, grad_offset);
}

int dlrm_sr_sgd_seek(dlrm_ctx* ctx, dlrm_sr_sgd* op, int64_t step) {
    CHECK_ARG(ctx && op, "dlrm_sr_sgd_seek: null ctx/optimizer");
    const int rc = hip_set(ctx);
    if (rc) return rc;
    return launch_sr_step_set(ctx, op->d_step, (uint64_t)step);
}

int dlrm_sr_sgd_step(dlrm_ctx* ctx, dlrm_sr_sgd* op, uint64_t* out) {
    CHECK_ARG(ctx && op && out, "dlrm_sr_sgd_step: null ctx/optimizer/out");
    int rc = hip_set(ctx);
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (rc == DLRM_OK) rc = ctx_hip(ctx, hipMemcpy(out, op->d_step, sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(sr step)");
    return rc;
}

// ----------------------------------------------------------------------- training step
int dlrm_step_fwd(dlrm_ctx* ctx, const dlrm_tables* tb, dlrm_indexer* ix, const void* indices, int itype,
                  int64_t table_stride, int index_base, int batch, const void* x, int64_t x_ld, void* out,
                  int64_t out_ld, int padding) {
    CHECK_ARG(ctx && tb && ix, "dlrm_step_fwd: null ctx/tables/indexer");
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, 1);
    if (rc) return rc;
    CHECK_ARG(tb->T == ix->T, "dlrm_step_fwd: indexer has %d tables, tables has %d", ix->T, tb->T);
    CHECK_ARG(batch <= ix->dev.cap, "dlrm_step_fwd: batch %d > indexer capacity %lld", batch, (long long)ix->dev.cap);
    const int d = tb->D, F = tb->T + 1;
    const int64_t P = (int64_t)F * (F - 1) / 2;
    CHECK_ARG(padding >= 0 && x_ld >= d && out_ld >= d + P + padding, "dlrm_step_fwd: leading dimensions too small");
    CHECK_ARG(batch == 0 || (x && out), "dlrm_step_fwd: null buffer");
    const IndexArgs ia{indices, itype, table_stride, index_base, batch, 1};
    const auto fused_fwd = [&] {
        return launch_lookup_interact_fwd(ctx, tb->d_desc, tb->aligned16, tb->T, tb->dtype, indices, itype, table_stride,
                                          index_base, 1, d, batch, x, x_ld, nullptr, 0, out, out_ld, padding,
                                          tb->h_desc.data());
    };
    BuildCaps caps{};
    // (a prepared build is kept where the fused forward can gather from it: otherwise the batch is built as any other)
    caps.prepared = ix->prepared && built_from(ix, indices, itype, table_stride, index_base, batch, 1) &&
                    lookup_fwd_supported(tb->aligned16, tb->T, tb->dtype, d, batch, x, x_ld, tb->h_desc.data());
    caps.step_fwd = step_fwd_supported(tb->aligned16, tb->T, tb->dtype, d, batch, x, x_ld, tb->h_desc.data());
    caps.step_split = step_split_supported(tb->aligned16, tb->T, tb->dtype, d, x, x_ld);
    const BuildPlan p = plan_build(BuildSite::StepFwd, shape_of(ix), batch, knobs(), caps);
    begin_build(ix, p);
    // built by the previous step's apply launch (dlrm_step_bwd_prepare) or by dlrm_indexer_prepare: the gather alone
    if (p.form == BuildForm::Kept) return fused_fwd();
    if (p.form == BuildForm::InForward) {
        rc = launch_step_fwd(ctx, tb->d_desc, tb->aligned16, tb->T, tb->dtype, indices, itype, table_stride, index_base, d,
                             batch, x, x_ld, out, out_ld, padding, ix->dev, tb->h_desc.data());
        if (rc) return rc;
        record_build(ix, p, ia);
        return DLRM_OK;
    }
    // no single-launch form for this shape: the fused forward and the plan's build -- after it on the ctx's stream,
    // or (large batches) before it on the side stream, which the main stream joins
    if (p.side) {
        rc = ensure_side(ctx);
        if (rc) return rc;
        rc = ctx_hip(ctx, hipEventRecord(ctx->ev_fork, ctx->stream), "hipEventRecord(fork)");
        if (rc == DLRM_OK) rc = ctx_hip(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0), "hipStreamWaitEvent(side)");
        if (rc == DLRM_OK) rc = run_build(ctx, ix, tb, p, ia);
        if (rc == DLRM_OK) rc = ctx_hip(ctx, hipEventRecord(ctx->ev_join, ctx->side), "hipEventRecord(join)");
        if (rc) return rc;
    }
    rc = fused_fwd();
    const int rj = p.side ? ctx_hip(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0), "hipStreamWaitEvent(main)")
                          : DLRM_OK;
    // the one refusal left to meet at run time: the fused forward's own
    if (rc == DLRM_E_UNSUPPORTED)
        return ctx_fail(ctx, DLRM_E_UNSUPPORTED,
                        "dlrm_step_fwd: no fused forward for this shape (16-B aligned rows and x, F <= 96 needed)");
    if (rc || rj) return rc ? rc : rj;
    if (!p.side) rc = run_build(ctx, ix, tb, p, ia);
    if (rc) return rc;
    record_build(ix, p, ia);
    return DLRM_OK;
}

// The training step's backward and apply under a rule: Descent (dlrm_step_bwd), the split rule on split-bf16 tables
// (dlrm_split_step_bwd), a sparse Adagrad rule (dlrm_adagrad_step_bwd; element-wise or row-wise by its handle) or the
// stochastic rule on bf16 tables (dlrm_sr_step_bwd).  An indexer remembers which rule, bound to which handle, stepped
// its once-hit rows, and only that one's apply completes the backward (check_completes).

// Whether the shape has the rule's split backward (once-hit rows stepped there): the shapes of the split kernels, the
// rule's second stream in 16-B aligned rows (the split rule's backward loads the low halves as 8-B or 16-B vectors,
// the element-wise Adagrad rule's its state rows as 16-B vectors), and the rule's once-hit write for the feature sizes
static bool has_split_bwd(const dlrm_tables* tb, const BoundRule& r, const void* x, int64_t x_ld) {
    return r.aligned16 && step_bwd_supported(r.kind, tb->aligned16, tb->T, tb->dtype, tb->D, x, x_ld);
}

static int step_bwd_impl(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_indexer* ix, const BoundRule& r, const void* indices,
                         int itype, int64_t table_stride, int index_base, int batch, const void* x, int64_t x_ld,
                         const void* dout, int64_t dout_ld, int padding, float* dx, int64_t dx_ld, float* dt,
                         int64_t dt_ld, unsigned flags, const PrepArgs* prep) {
    const char* const fn = kRules[r.kind].step_fn;
    int rc = check_indices(ctx, tb, indices, itype, table_stride, batch, 1);
    if (rc == DLRM_OK) rc = check_rule(ctx, tb, r, fn);  // (the argument errors of the rule's update)
    if (rc) return rc;
    const int d = tb->D, F = tb->T + 1;
    const int64_t P = (int64_t)F * (F - 1) / 2;
    CHECK_ARG(padding >= 0 && x_ld >= d && dout_ld >= d + P + padding && dx_ld >= d && dt_ld >= (int64_t)F * d,
              "%s: leading dimensions too small", fn);
    CHECK_ARG(batch == 0 || (x && dout && dx && dt), "%s: null buffer", fn);
    if (!built_from(ix, indices, itype, table_stride, index_base, batch, 1))
        return ctx_fail(ctx, DLRM_E_STATE, "%s: the indexer was not built by dlrm_step_fwd from these indices", fn);
    CHECK_ARG(flags != (DLRM_STEP_BWD_ONLY | DLRM_STEP_APPLY_ONLY), "%s: flags %u", fn, flags);
    rc = ensure_partials(ctx, ix, tb->D);
    if (rc) return rc;
    // the split backward (once-hit rows updated there) where the shape has it; otherwise the
    // gather backward writes every dt row and the apply takes a split indexer's once-hit rows too
    const bool split_bwd = ix->split && has_split_bwd(tb, r, x, x_ld);
    if (flags & DLRM_STEP_APPLY_ONLY) {
        // the apply of a split build only completes a backward that stepped the once-hit rows
        if (split_bwd && !ix->singles_done)
            return ctx_fail(ctx, DLRM_E_STATE, "%s(APPLY_ONLY): no backward has run on this build", fn);
        rc = check_completes(ctx, ix, r, fn, "(APPLY_ONLY)");
    } else if (split_bwd) {
        // a second backward on one build would step its once-hit rows twice
        if (ix->singles_done)
            return ctx_fail(ctx, DLRM_E_STATE,
                            "%s: this build's once-hit rows were already stepped (one backward per "
                            "dlrm_step_fwd)", fn);
        CHECK_ARG((uintptr_t)dx % 16 == 0 && (uintptr_t)dt % 16 == 0 && dx_ld % 4 == 0 && dt_ld % 4 == 0,
                  "%s: dx and dt must be 16-B aligned with leading dimensions divisible by 4", fn);
        // (the stochastic rule: reads the handle's step word; the launch that runs the apply advances it)
        rc = launch_step_bwd(ctx, tb->d_desc, tb->T, tb->dtype, indices, itype, table_stride, index_base, d, batch, x,
                             x_ld, dout, dout_ld, dx, dx_ld, dt, dt_ld, ix->dev, r);
        if (rc == DLRM_OK) {
            ix->singles_done = true;
            ix->singles_rule = r.kind;
            ix->singles_handle = r.handle;
        }
    } else {
        rc = launch_interact_bwd_gather(ctx, tb->d_desc, tb->aligned16, tb->T, tb->dtype, indices, itype, table_stride,
                                        index_base, 1, d, batch, x, x_ld, dout, dout_ld, dx, dx_ld, dt, dt_ld, nullptr);
    }
    if (rc || (flags & DLRM_STEP_BWD_ONLY)) return rc;
    // once-hit rows: updated by the split backward, else by this apply (an unsplit indexer lists
    // them as chunks)
    const SinglesArgs sa{(ix->split && !split_bwd) ? ix->dev.single : nullptr, indices, itype, table_stride,
                         index_base, batch};
    return kRules[r.kind].step_apply(ctx, ix->dev, tb->d_desc, tb->aligned16 && r.aligned16, tb->T, tb->D, tb->dtype, 1,
                                     (int64_t)batch, dt, DLRM_F32, dt_ld, d, r, sa, prep);
}

static int step_bwd_prepare_impl(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_indexer* ix, const BoundRule& r,
                                 const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                                 const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding, float* dx,
                                 int64_t dx_ld, float* dt, int64_t dt_ld, dlrm_indexer* next, const void* next_indices,
                                 unsigned flags) {
    const char* const fn = kRules[r.kind].step_fn;
    CHECK_ARG(next && next != ix, "%s_prepare: null or shared indexer", fn);
    CHECK_ARG(next->T == tb->T && batch <= next->dev.cap, "%s_prepare: next indexer too small", fn);
    int rc = check_indices(ctx, tb, next_indices, itype, table_stride, batch, 1);
    if (rc) return rc;
    // the next batch's build runs as extra workgroups of this step's apply launch: the step
    // forward's split build (the same parts), so the next dlrm_step_fwd only gathers
    BuildCaps caps{};
    caps.split_bwd = has_split_bwd(tb, r, x, x_ld);
    caps.bwd_only = (flags & DLRM_STEP_BWD_ONLY) != 0;
    caps.idx_vec32 = idx_vec32(next_indices, itype, table_stride);
    const BuildPlan p = plan_build(BuildSite::InApply, shape_of(next), batch, knobs(), caps);
    // no pipelined form for this shape: the plain step (the next forward builds); BWD_ONLY: the next build rides on
    // the apply launch
    if (p.form == BuildForm::None)
        return step_bwd_impl(ctx, tb, ix, r, indices, itype, table_stride, index_base, batch, x, x_ld, dout, dout_ld,
                             padding, dx, dx_ld, dt, dt_ld, flags, nullptr);
    begin_build(next, p);
    // the wave build: 2^vshift parts per table, one wave each (4 per workgroup)
    const PrepArgs pa{next->dev, tb->d_desc, tb->T, next_indices, itype, table_stride, index_base, batch,
                      err_word(ctx, next, p.err)};
    rc = step_bwd_impl(ctx, tb, ix, r, indices, itype, table_stride, index_base, batch, x, x_ld, dout, dout_ld, padding,
                       dx, dx_ld, dt, dt_ld, flags, &pa);
    if (rc) return rc;
    record_build(next, p, IndexArgs{next_indices, itype, table_stride, index_base, batch, 1});
    return DLRM_OK;
}

// The public pairs: each binds its rule and passes it down.  (The stochastic rule's handle's step word is read by both
// launches of a step and advanced after the one that runs the apply.)
#define STEP_ARGS                                                                                                     \
    const void *indices, int itype, int64_t table_stride, int index_base, int batch, const void *x, int64_t x_ld,     \
        const void *dout, int64_t dout_ld, int padding, float *dx, int64_t dx_ld, float *dt, int64_t dt_ld
#define STEP_PASS indices, itype, table_stride, index_base, batch, x, x_ld, dout, dout_ld, padding, dx, dx_ld, dt, dt_ld

int dlrm_step_bwd(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_indexer* ix, STEP_ARGS, float lr, unsigned flags) {
    CHECK_ARG(ctx && tb && ix, "dlrm_step_bwd: null ctx/tables/indexer");
    return step_bwd_impl(ctx, tb, ix, bind_rule(lr), STEP_PASS, flags, nullptr);
}

int dlrm_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_indexer* ix, STEP_ARGS, float lr, dlrm_indexer* next,
                          const void* next_indices, unsigned flags) {
    CHECK_ARG(ctx && tb && ix, "dlrm_step_bwd_prepare: null or shared indexer");
    return step_bwd_prepare_impl(ctx, tb, ix, bind_rule(lr), STEP_PASS, next, next_indices, flags);
}

int dlrm_split_step_bwd(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_split_sgd* op, dlrm_indexer* ix, STEP_ARGS, float lr,
                        unsigned flags) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_split_step_bwd: null ctx/tables/optimizer/indexer");
    return step_bwd_impl(ctx, tb, ix, bind_rule(op, lr), STEP_PASS, flags, nullptr);
}

int dlrm_split_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_split_sgd* op, dlrm_indexer* ix, STEP_ARGS,
                                float lr, dlrm_indexer* next, const void* next_indices, unsigned flags) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_split_step_bwd_prepare: null ctx/tables/optimizer/indexer");
    return step_bwd_prepare_impl(ctx, tb, ix, bind_rule(op, lr), STEP_PASS, next, next_indices, flags);
}

int dlrm_adagrad_step_bwd(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_adagrad* op, dlrm_indexer* ix, STEP_ARGS, float lr,
                          float eps, unsigned flags) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_adagrad_step_bwd: null ctx/tables/optimizer/indexer");
    if (op->stochastic)  // (nothing launched or written; the handle's step word stays)
        return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "dlrm_adagrad_step_bwd: no fused training step with a stochastic handle "
                        "(dlrm_adagrad_create_sr): dlrm_adagrad_update steps its tables");
    return step_bwd_impl(ctx, tb, ix, bind_rule(op, lr, eps), STEP_PASS, flags, nullptr);
}

int dlrm_adagrad_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_adagrad* op, dlrm_indexer* ix, STEP_ARGS,
                                  float lr, float eps, dlrm_indexer* next, const void* next_indices, unsigned flags) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_adagrad_step_bwd_prepare: null ctx/tables/optimizer/indexer");
    if (op->stochastic)  // (nothing launched or written; the handle's step word stays)
        return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "dlrm_adagrad_step_bwd_prepare: no fused training step with a stochastic handle "
                        "(dlrm_adagrad_create_sr): dlrm_adagrad_update steps its tables");
    return step_bwd_prepare_impl(ctx, tb, ix, bind_rule(op, lr, eps), STEP_PASS, next, next_indices, flags);
}

int dlrm_sr_step_bwd(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_sr_sgd* op, dlrm_indexer* ix, STEP_ARGS, float lr,
                     unsigned flags) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_sr_step_bwd: null ctx/tables/optimizer/indexer");
    return step_bwd_impl(ctx, tb, ix, bind_rule(op, lr), STEP_PASS, flags, nullptr);
}

int dlrm_sr_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_sr_sgd* op, dlrm_indexer* ix, STEP_ARGS, float lr,
                             dlrm_indexer* next, const void* next_indices, unsigned flags) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_sr_step_bwd_prepare: null ctx/tables/optimizer/indexer");
    return step_bwd_prepare_impl(ctx, tb, ix, bind_rule(op, lr), STEP_PASS, next, next_indices, flags);
}
// (a seeded handle's pair: dlrm_adagrad_step_bwd's refusal of such a handle stays as it is)
int dlrm_sr_adagrad_step_bwd(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_adagrad* op, dlrm_indexer* ix, STEP_ARGS, float lr,
                             float eps, unsigned flags) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_sr_adagrad_step_bwd: null ctx/tables/optimizer/indexer");
    CHECK_ARG(op->stochastic, "dlrm_sr_adagrad_step_bwd: the handle has no seed (dlrm_adagrad_create_sr makes one that "
              "has; dlrm_adagrad_step_bwd takes this one)");
    return step_bwd_impl(ctx, tb, ix, bind_rule(op, lr, eps), STEP_PASS, flags, nullptr);
}

int dlrm_sr_adagrad_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tb, dlrm_adagrad* op, dlrm_indexer* ix, STEP_ARGS,
                                     float lr, float eps, dlrm_indexer* next, const void* next_indices,
                                     unsigned flags) {
    CHECK_ARG(ctx && tb && op && ix, "dlrm_sr_adagrad_step_bwd_prepare: null ctx/tables/optimizer/indexer");
    CHECK_ARG(op->stochastic, "dlrm_sr_adagrad_step_bwd_prepare: the handle has no seed (dlrm_adagrad_create_sr makes "
              "one that has; dlrm_adagrad_step_bwd_prepare takes this one)");
    return step_bwd_prepare_impl(ctx, tb, ix, bind_rule(op, lr, eps), STEP_PASS, next, next_indices, flags);
}
#undef STEP_ARGS
#undef STEP_PASS

// ---- diagnostics: a native backtrace on a fatal signal (SIGSEGV / SIGBUS / SIGABRT), written to
// stderr before the previous handler runs (Python's faulthandler then prints the Python stack).
static struct sigaction g_prev[3];
static const int g_sigs[3] = {SIGSEGV, SIGBUS, SIGABRT};
static void fatal_trace(int sig, siginfo_t* si, void* uc) {
    static const char head[] = "\n[dlrm] fatal signal, native backtrace (innermost first):\n";
    (void)!write(2, head, sizeof head - 1);
    char line[96];
    const int n0 = snprintf(line, sizeof line, "[dlrm] signal %d, fault address %p\n", sig, si ? si->si_addr : nullptr);
    if (n0 > 0) (void)!write(2, line, (size_t)n0);
    void* fr[64];
    const int n = backtrace(fr, 64);
    backtrace_symbols_fd(fr, n, 2);
    for (int k = 0; k < 3; ++k)
        if (g_sigs[k] == sig) {
            sigaction(sig, &g_prev[k], nullptr);
            if (g_prev[k].sa_flags & SA_SIGINFO) {
                if (g_prev[k].sa_sigaction) {
                    g_prev[k].sa_sigaction(sig, si, uc);
                    return;
                }
            } else if (g_prev[k].sa_handler != SIG_DFL && g_prev[k].sa_handler != SIG_IGN) {
                g_prev[k].sa_handler(sig);
                return;
            }
        }
    signal(sig, SIG_DFL);
    raise(sig);
}

int dlrm_debug_fatal_trace(int on) {
    if (on == 2) {  // report who owns the handlers now (dladdr of the installed function), then arm
        for (int k = 0; k < 3; ++k) {
            struct sigaction cur;
            if (sigaction(g_sigs[k], nullptr, &cur) != 0) continue;
            void* fn = (cur.sa_flags & SA_SIGINFO) ? (void*)cur.sa_sigaction : (void*)cur.sa_handler;
            Dl_info di;
            memset(&di, 0, sizeof di);
            const bool named = fn && dladdr(fn, &di) != 0;
            fprintf(stderr, "[dlrm] signal %d handler %p (%s in %s)\n", g_sigs[k], fn,
                    named && di.dli_sname ? di.dli_sname : "?", named && di.dli_fname ? di.dli_fname : "?");
        }
        fflush(stderr);
    }
    if (on) {  // an alternate signal stack for this thread: a stack overflow is a SIGSEGV too
        static char* alt = nullptr;
        if (!alt) alt = (char*)malloc(1 << 20);
        if (alt) {
            stack_t ss;
            memset(&ss, 0, sizeof ss);
            ss.ss_sp = alt;
            ss.ss_size = 1 << 20;
            (void)sigaltstack(&ss, nullptr);
        }
    }
    for (int k = 0; k < 3; ++k) {
        if (on) {
            struct sigaction sa, old;
            memset(&sa, 0, sizeof sa);
            sa.sa_sigaction = fatal_trace;
            sa.sa_flags = SA_SIGINFO | SA_RESETHAND | SA_ONSTACK;
            sigemptyset(&sa.sa_mask);
            if (sigaction(g_sigs[k], &sa, &old) != 0) return DLRM_E_ARG;
            // (re-arming keeps the handler found the first time: chaining to ourselves would recurse)
            if (!((old.sa_flags & SA_SIGINFO) && old.sa_sigaction == fatal_trace)) g_prev[k] = old;
        } else {
            sigaction(g_sigs[k], &g_prev[k], nullptr);
        }
    }
    return DLRM_OK;
}

}  // extern "C"
