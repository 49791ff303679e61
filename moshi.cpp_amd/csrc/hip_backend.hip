// hip_backend.hip — the MI355X ("ROCm<N>") ggml backend: device registry, pooled device buffers,
// batched small uploads, and the graph planner / executor.
//
// Execution model (SURVEY.md §7 "hard parts": ~4.5 k ggml nodes per frame vs. a sub-millisecond roofline
// budget, so per-node dispatch is impossible):
//   * ggml_backend_graph_compute() turns a cgraph into a *plan*: an ordered list of kernel launches in
//     which the hot node sequences (norm -> mat-vec, gated FFN, residual add, the whole single-token
//     attention block, the 17-stream embedding sum) are matched and replaced by the fused kernels of
//     hip_kernels_fused.hip; everything else falls back to one generic kernel per node. The planner is
//     build_plan: one match_* function per node pattern, one pass_* function per fusion that claims the
//     matched nodes under one rule (claim), the passes in the order of the fusion_passes list, then the
//     post-passes that emit the attention groups, lay the steps out and merge runs into persistent chains.
//   * plans of cached graphs (Temporal / Depth / Mimi graphs are built once by the caller and replayed
//     every frame, src/context.h:538-544) are captured into a hipGraph and replayed with one
//     hipGraphLaunch; throw-away scratch graphs (src/context.h:628-653) are launched directly.
//   * the ~40 scalar tensor_set calls per frame (lm_utils.h:172-182) are queued in pinned host memory
//     and scattered by one kernel at the next compute / read-back.
// ggml semantics preserved: every non-view tensor has its own storage, execution order = node order,
// results are visible to tensor_get when graph_compute returns (stream-ordered, tensor_get synchronises).
#include "hip_common.h"
#include "ggml-cpu.h"

#include <string.h>

#include <algorithm>
#include <functional>
#include <deque>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

// ---------------------------------------------------------------------------------------------------
// per-device context
// ---------------------------------------------------------------------------------------------------
#define UPLOAD_SLOTS       8
#define UPLOAD_BLOB_BYTES  (64 * 1024)
#define UPLOAD_MAX_DESCS   1024
#define READBACK_PINNED_BYTES (64 * 1024)
#define AGET_SLOTS 64
#define AGET_SLOT_BYTES 256
#define UPLOAD_SMALL_MAX   16384   // the 7.7 KB PCM frame rides the batched path too (a pageable hipMemcpy + sync otherwise)

struct plan_t;

struct upload_slot {
    char * blob = nullptr;            // pinned, device-mapped
    upload_desc * descs = nullptr;    // pinned, device-mapped
    hipEvent_t done = nullptr;
    bool in_flight = false;
};

struct hip_ctx {
    int device = 0;
    std::string name, description;
    hipStream_t stream = nullptr;
    int flags = 0;
    int max_columns = 16;        // ggml_backend_mi355x_set_max_columns: the widest B-column sampler graph planned as one launch
    int float_acc = 0;           // ggml_backend_mi355x_set_float_accumulate: 1 = BF16 / F16 weights against 2..64 rows take the float-accumulating mat-mul
    bool no_capture = false;     // ggml_backend_mi355x_set_capture(.., 0): plans of repeated graphs are reused but not captured into hipGraphs
    ggml_mi355x_stats stats = {};
    // pooled allocations: size class -> free pointers
    std::map<size_t, std::vector<void *>> pool;
    // batched uploads
    upload_slot slots[UPLOAD_SLOTS];
    int cur_slot = 0;
    int n_pending = 0;
    size_t pending_bytes = 0;
    // flag 8: per-launch timing of the dominant kernel
    mv_profile prof = { nullptr, 0, 0 };
    double prof_seconds = 0; int64_t prof_launches = 0, prof_bytes = 0;
    double prof_seconds_v[3] = { 0, 0, 0 }; int64_t prof_launches_v[3] = { 0, 0, 0 }, prof_bytes_v[3] = { 0, 0, 0 };   // the same, by kernel variant
    double prof_chain_seconds = 0; int64_t prof_chain_launches = 0, prof_chain_bytes = 0, prof_chain_phases = 0;   // persistent chain launches (matvec_chain_kernel), stream events
    hipEvent_t chain_ev[2] = { nullptr, nullptr };
    // cached plans keyed by cgraph pointer
    std::unordered_map<const ggml_cgraph *, plan_t *> plans;
    uint64_t orphan_clock = 0;
    // device-visible error word in pinned host memory: kernels with bounded waits raise it instead of hanging
    volatile unsigned * err_host = nullptr;
    unsigned * err_dev = nullptr;
    char * readback = nullptr;   // pinned staging for small device -> host reads
    // stream-ordered small read-backs (ggml_backend_tensor_get_async): staged in pinned slots, handed to the caller's memory by the synchronize / event
    // wait that covers them
    struct async_get { void * dst; size_t size; int slot; uint64_t seq; };
    char * aget_pinned = nullptr;
    std::deque<async_get> aget_pending;
    uint64_t aget_seq = 0;
    bool in_use = false;         // stream contexts only: handed out by ggml_backend_mi355x_init_stream, returned by ggml_backend_free
    int usable_cus = 0;          // compute units this context's stream may use: the device's count, or MI355X_STREAM_CUS of them (CU-masked stream)
    ggml_backend_device dev_obj;
};

static std::vector<hip_ctx *> & contexts() { static std::vector<hip_ctx *> v; return v; }
// additional command streams on a device (ggml_backend_mi355x_init_stream): a full context of its own - stream, upload slots, pool, plan cache -
// on the same GPU, so graphs submitted through it overlap with the device's first stream. Not listed by the registry.
static std::vector<hip_ctx *> & stream_contexts() { static std::vector<hip_ctx *> v; return v; }

static void set_device(hip_ctx * c) { HIP_CHECK(hipSetDevice(c->device)); }

static void ctx_init_lazy(hip_ctx * c) {
    if (c->stream) return;
    set_device(c);
    {
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, c->device));
        c->usable_cus = prop.multiProcessorCount;
        // MI355X_STREAM_CUS=n: confine this backend's stream to n compute units (hipExtStreamCreateWithCUMask with bits 0 .. n - 1 of the mask set; which
        // physical CUs / XCDs those bits name is the runtime's mapping and is not assumed here) - the shape of a CU-masked or partitioned deployment. Kernels
        // whose workgroups wait for each other (persistent chains, the fused attention + out_proj launch, split attention) are planned against this NUMBER
        // and fall back to plain launches when their grid cannot be resident (build_plan). Unlike the default stream below, a CU-masked stream is created
        // WITHOUT hipStreamNonBlocking (the call takes no flags): it synchronises implicitly with the NULL stream - a diagnostic / test shape, not a fast path.
        const char * e = getenv("MI355X_STREAM_CUS");
        const int lim = e ? atoi(e) : 0;
        if (lim > 0 && lim < prop.multiProcessorCount) {
            std::vector<uint32_t> mask((size_t) (prop.multiProcessorCount + 31) / 32, 0u);
            for (int i = 0; i < lim; i++) mask[(size_t) i / 32] |= 1u << (i % 32);
            HIP_CHECK(hipExtStreamCreateWithCUMask(&c->stream, (uint32_t) mask.size(), mask.data()));
            c->usable_cus = lim;
        }
    }
    if (!c->stream) HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (auto & s : c->slots) {
        HIP_CHECK(hipHostMalloc((void **) &s.blob, UPLOAD_BLOB_BYTES, hipHostMallocMapped));
        HIP_CHECK(hipHostMalloc((void **) &s.descs, UPLOAD_MAX_DESCS * sizeof(upload_desc), hipHostMallocMapped));
        HIP_CHECK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    HIP_CHECK(hipHostMalloc((void **) &c->readback, READBACK_PINNED_BYTES, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void **) &c->aget_pinned, AGET_SLOTS * AGET_SLOT_BYTES, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void **) &c->err_host, 64, hipHostMallocMapped));
    c->err_host[0] = 0u;
    HIP_CHECK(hipHostGetDevicePointer((void **) &c->err_dev, (void *) c->err_host, 0));
}

static void check_device_error(hip_ctx * c) {
    if (c->err_host && c->err_host[0] != 0u)
        GGML_ABORT("mi355x backend: a kernel gave up a bounded wait (code %u: 1 = split attention head barrier, 2 = chain engine hand-off, 3 = stream engine hand-off); results are invalid", c->err_host[0]);
}

// ---- pool -----------------------------------------------------------------------------------------
static size_t size_class(size_t n) {
    if (n > ((size_t) 64 << 20)) return 0;   // large: not pooled
    size_t c = 256;
    while (c < n) c <<= 1;
    return c;
}
// MI355X_POISON=1 (diagnosis): every buffer and workspace handed out is first filled with 0xFF bytes (NaN as F32 / BF16 / F16, -1 as I32), so
// that a kernel reading memory nobody wrote shows up as NaNs or wild indices in the parity tests instead of passing on leftover zeros
static void * pool_poison(hip_ctx * c, void * p, size_t n) {
    static const bool poison = getenv("MI355X_POISON") != nullptr;
    if (poison && p) { HIP_CHECK(hipMemsetAsync(p, 0xFF, n, c->stream)); HIP_CHECK(hipStreamSynchronize(c->stream)); }
    return p;
}
// MI355X_GUARD=1 (diagnosis): every allocation sits between two 4 KB zones filled with 0xA5; they are checked when the allocation is
// returned - a kernel writing just outside its buffer aborts the process with the offending size instead of corrupting a neighbour
#define GUARD_BYTES 4096
static bool guard_mode() { static const bool g = getenv("MI355X_GUARD") != nullptr; return g; }
static void guard_fill(hip_ctx * c, char * user, size_t actual) {
    HIP_CHECK(hipMemsetAsync(user - GUARD_BYTES, 0xA5, GUARD_BYTES, c->stream));
    HIP_CHECK(hipMemsetAsync(user + actual, 0xA5, GUARD_BYTES, c->stream));
}
static void guard_check(hip_ctx * c, char * user, size_t actual) {
    static std::vector<unsigned char> h(2 * GUARD_BYTES);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(h.data(), user - GUARD_BYTES, GUARD_BYTES, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h.data() + GUARD_BYTES, user + actual, GUARD_BYTES, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < 2 * GUARD_BYTES; i++)
        if (h[i] != 0xA5) GGML_ABORT("mi355x: guard zone %s a %zu-byte allocation was overwritten (offset %zu)", i < GUARD_BYTES ? "before" : "after", actual, i % GUARD_BYTES);
}
static void * pool_alloc(hip_ctx * c, size_t n, size_t * actual) {
    set_device(c);
    const size_t cls = size_class(n ? n : 1);
    if (cls) {
        auto & fl = c->pool[cls];
        *actual = cls;
        if (!fl.empty()) { void * p = fl.back(); fl.pop_back(); if (guard_mode()) guard_fill(c, (char *) p, *actual); return pool_poison(c, p, *actual); }
    } else *actual = n;
    void * p = nullptr;
    hipError_t e = hipMalloc(&p, *actual + (guard_mode() ? 2 * GUARD_BYTES : 0));
    if (e != hipSuccess) { fprintf(stderr, "mi355x: hipMalloc(%zu) failed: %s\n", *actual, hipGetErrorString(e)); return nullptr; }
    if (guard_mode()) { p = (char *) p + GUARD_BYTES; guard_fill(c, (char *) p, *actual); }
    return pool_poison(c, p, *actual);
}
static void pool_free(hip_ctx * c, void * p, size_t actual) {
    if (!p) return;
    if (guard_mode()) guard_check(c, (char *) p, actual);
    const size_t cls = size_class(actual);
    if (cls && cls == actual) { c->pool[cls].push_back(p); return; }
    set_device(c);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipFree(guard_mode() ? (char *) p - GUARD_BYTES : (char *) p));
}

// ---- batched uploads -------------------------------------------------------------------------------
static void flush_uploads(hip_ctx * c) {
    if (c->n_pending == 0) return;
    upload_slot & s = c->slots[c->cur_slot];
    k_scatter_uploads(c->stream, s.descs, s.blob, c->n_pending);
    HIP_CHECK(hipEventRecord(s.done, c->stream));
    s.in_flight = true;
    c->stats.uploads_batched += c->n_pending;
    c->n_pending = 0;
    c->pending_bytes = 0;
    c->cur_slot = (c->cur_slot + 1) % UPLOAD_SLOTS;
    upload_slot & n = c->slots[c->cur_slot];
    if (n.in_flight) { HIP_CHECK(hipEventSynchronize(n.done)); n.in_flight = false; }
}

static void queue_upload(hip_ctx * c, void * dst, const void * src, size_t size) {
    const size_t padded = GGML_PAD(size, 16);
    if (c->n_pending >= UPLOAD_MAX_DESCS || c->pending_bytes + padded > UPLOAD_BLOB_BYTES) flush_uploads(c);
    // the scatter kernel copies all descriptors of a batch concurrently: a second write to bytes already pending (a state's zero fill
    // followed by its first value, say) must not share a batch with the first, or the older data may land last
    for (int i = 0; i < c->n_pending; i++) {
        const upload_desc & d = c->slots[c->cur_slot].descs[i];
        if ((char *) dst < d.dst + d.size && d.dst < (char *) dst + size) { flush_uploads(c); break; }
    }
    upload_slot & s = c->slots[c->cur_slot];
    memcpy(s.blob + c->pending_bytes, src, size);
    s.descs[c->n_pending] = { (char *) dst, (uint32_t) c->pending_bytes, (uint32_t) size };
    c->n_pending++;
    c->pending_bytes += padded;
}

// ---------------------------------------------------------------------------------------------------
// buffers
// ---------------------------------------------------------------------------------------------------
struct hip_buffer_ctx { hip_ctx * c; size_t actual; };

// the stream has reached (at least) read-back `upto`: copy the staged bytes to where the callers asked for them
static void deliver_async_gets(hip_ctx * c, uint64_t upto) {
    while (!c->aget_pending.empty() && c->aget_pending.front().seq <= upto) {
        const hip_ctx::async_get & g = c->aget_pending.front();
        memcpy(g.dst, c->aget_pinned + (size_t) g.slot * AGET_SLOT_BYTES, g.size);
        c->aget_pending.pop_front();
    }
}

static void evict_plans_of_buffer(hip_ctx * c, const ggml_backend_buffer * b);

static void hip_buf_free(ggml_backend_buffer_t b) {
    hip_buffer_ctx * bc = (hip_buffer_ctx *) b->context;
    flush_uploads(bc->c);
    // plans (captured hipGraphs with baked pointers, pool workspaces) must not silently outlive the memory they address - on any stream of the device
    evict_plans_of_buffer(bc->c, b);
    for (hip_ctx * o : contexts()) if (o != bc->c && o->device == bc->c->device) evict_plans_of_buffer(o, b);
    for (hip_ctx * o : stream_contexts()) if (o != bc->c && o->device == bc->c->device) evict_plans_of_buffer(o, b);
    pool_free(bc->c, b->base, bc->actual);
    delete bc;
    delete b;
}
static void hip_buf_set(ggml_backend_buffer_t b, struct ggml_tensor * t, const void * data, size_t offset, size_t size) {
    hip_ctx * c = ((hip_buffer_ctx *) b->context)->c;
    set_device(c);
    if (size <= UPLOAD_SMALL_MAX && !(c->flags & 4)) { queue_upload(c, (char *) t->data + offset, data, size); return; }
    flush_uploads(c);
    HIP_CHECK(hipMemcpyAsync((char *) t->data + offset, data, size, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
static void hip_buf_get(ggml_backend_buffer_t b, const struct ggml_tensor * t, void * data, size_t offset, size_t size) {
    hip_ctx * c = ((hip_buffer_ctx *) b->context)->c;
    set_device(c);
    flush_uploads(c);
    if (size <= READBACK_PINNED_BYTES) {
        // small read-backs (token ids, one PCM frame) land in a pinned staging buffer: a pageable destination makes the runtime
        // pin / stage it on every call
        HIP_CHECK(hipMemcpyAsync(c->readback, (const char *) t->data + offset, size, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        memcpy(data, c->readback, size);
    } else {
        HIP_CHECK(hipMemcpyAsync(data, (const char *) t->data + offset, size, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    deliver_async_gets(c, c->aget_seq);
    check_device_error(c);
}
static void hip_buf_memset(ggml_backend_buffer_t b, struct ggml_tensor * t, uint8_t v, size_t offset, size_t size) {
    hip_ctx * c = ((hip_buffer_ctx *) b->context)->c;
    set_device(c);
    flush_uploads(c);
    HIP_CHECK(hipMemsetAsync((char *) t->data + offset, v, size, c->stream));
}
static void hip_buf_clear(ggml_backend_buffer_t b, uint8_t v) {
    hip_ctx * c = ((hip_buffer_ctx *) b->context)->c;
    set_device(c);
    flush_uploads(c);
    HIP_CHECK(hipMemsetAsync(b->base, v, b->size, c->stream));
}

static ggml_backend_buffer_t hip_alloc_buffer(ggml_backend_t backend, size_t size) {
    hip_ctx * c = (hip_ctx *) backend->context;
    ctx_init_lazy(c);
    size_t actual = 0;
    void * p = pool_alloc(c, size, &actual);
    if (!p) return NULL;
    auto * b = new ggml_backend_buffer;
    b->iface = { hip_buf_free, hip_buf_memset, hip_buf_set, hip_buf_get, hip_buf_clear };
    b->device = &c->dev_obj;
    b->base = p;
    b->size = size;
    b->context = new hip_buffer_ctx{ c, actual };
    b->is_host = false;
    return b;
}

// ---------------------------------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------------------------------
typedef std::function<void(hipStream_t)> step_fn;
// one launch of a plan. Block mat-vecs keep their arguments visible: runs of consecutive small ones are merged into persistent chain launches
// (hip_chain.hip) once the whole plan is laid out
struct pstep {
    step_fn fn; bool is_mv = false; mv_args mv;
    chain_plan * chain = nullptr;   // a persistent chain launch (timed on its own in profile mode)
    const vq_level_args * vq = nullptr;   // one RVQ encode level (k_vq_level): consecutive levels of a stack may become one launch (k_vq_chain_*)
    // a step that reads nothing a launch of this graph writes (the RoPE table of add(positions, offset)) and writes [hoist_dst, + hoist_bytes): it may move in
    // front of a neighbouring mat-vec whose operands it does not overlap, so that the mat-vec stays next to the steps it chains with
    const char * hoist_dst = nullptr; size_t hoist_bytes = 0;
    template <typename F> pstep(F f) : fn(std::move(f)) { memset(&mv, 0, sizeof(mv)); }
    pstep(const mv_args & a) : fn([a](hipStream_t s) { k_matvec(s, a); }), is_mv(true), mv(a) {}
    // a step that is not a mat-vec but may be taken into a persistent step program next to its neighbours (mv.special): it keeps its own launch otherwise
    template <typename F> static pstep special_step(F f, int special, const attn_args * at, const lowrank_embed_args * lr, const sample_args * smp = nullptr) {
        pstep st(std::move(f));
        st.is_mv = true; st.mv.special = special; st.mv.attn = at; st.mv.lr = lr; st.mv.smp = smp;
        return st;
    }
};

struct plan_t {
    std::vector<pstep> steps;
    std::vector<chain_plan *> chains;
    std::vector<std::pair<void *, size_t>> workspaces;
    std::vector<std::unique_ptr<attn_args>> attn_copies;
    std::vector<std::unique_ptr<lowrank_embed_args>> lowrank_copies;
    std::vector<std::unique_ptr<sample_args>> sampler_copies;
    std::vector<std::unique_ptr<vq_level_args>> vq_copies;
    std::vector<vq_chain_plan *> vq_chains;
    std::vector<std::unique_ptr<conv_scatter>> scatter_slots;   // see emitter::scatter_of
    std::vector<const ggml_backend_buffer *> buffers;   // every buffer a node / leaf of the planned graph lives in: freeing one orphans the plan
    uint64_t orphan_seq = 0;                            // != 0: a buffer of the planned graph has been freed since (see evict_plans_of_buffer)
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    uint64_t hash = 0;
    int n_nodes = 0, n_fused = 0, n_chained = 0, n_attn_folded = 0, n_step_programs = 0, n_vq_chained = 0, n_attn_block_launches = 0, n_attn_block_jobs = 0, n_generic_attn_nodes = 0, n_ring_copy_launches = 0, n_ring_copy_jobs = 0, n_attn_row_launches = 0, n_attn_row_jobs = 0, n_attn_row_rows = 0, n_cross_block_launches = 0, n_cross_block_jobs = 0, n_float_batched_mms = 0, n_float_acc_mms = 0, n_pass_input_launches = 0, n_pass_input_rows = 0, n_convtr_column_groups = 0, n_codec_attn_launches = 0, n_vq_column_levels = 0, n_code_gather_columns = 0, n_state_copy_launches = 0, n_state_copy_jobs = 0;
};

static void plan_free(hip_ctx * c, plan_t * p) {
    if (p->exec) (void) hipGraphExecDestroy(p->exec);
    if (p->graph) (void) hipGraphDestroy(p->graph);
    for (auto & w : p->workspaces) pool_free(c, w.first, w.second);
    for (chain_plan * ch : p->chains) k_chain_free(ch);
    for (vq_chain_plan * vc : p->vq_chains) k_vq_chain_free(vc);
    delete p;
}

// A plan bakes device addresses into its launch arguments. When a buffer it touches is freed (moshi_hot_free, a scratch context going away) the
// plan becomes an ORPHAN: it is only ever used again if a graph with the same full hash - same tensor descriptors at the same host addresses with
// the same device addresses - is submitted under the same cgraph pointer (the scratch protocol of src/context.h:628-653 rebuilds structurally
// identical graphs in place: one plan then serves every chunk of a prompt prefill). Anything else at that address replaces it, and at most
// MAX_ORPHANS are kept (oldest first out), so plans of freed models do not pile up with their pool workspaces.
#define MAX_ORPHANS 8
static void collect_plan_buffers(plan_t * p, const ggml_cgraph * g) {
    p->buffers.clear();
    auto note = [&](const ggml_tensor * t) {
        const ggml_backend_buffer * b = t->buffer ? t->buffer : (t->view_src ? t->view_src->buffer : nullptr);
        if (b && std::find(p->buffers.begin(), p->buffers.end(), b) == p->buffers.end()) p->buffers.push_back(b);
    };
    for (int i = 0; i < g->n_nodes; i++) note(g->nodes[i]);
    for (int i = 0; i < g->n_leafs; i++) note(g->leafs[i]);
}
static void evict_plans_of_buffer(hip_ctx * c, const ggml_backend_buffer * b) {
    for (auto & kv : c->plans) {
        plan_t * p = kv.second;
        if (p->orphan_seq || std::find(p->buffers.begin(), p->buffers.end(), b) == p->buffers.end()) continue;
        p->orphan_seq = ++c->orphan_clock;
        p->buffers.clear();
    }
    for (;;) {   // bound the orphans
        int n = 0; auto oldest = c->plans.end();
        for (auto it = c->plans.begin(); it != c->plans.end(); ++it)
            if (it->second->orphan_seq) { n++; if (oldest == c->plans.end() || it->second->orphan_seq < oldest->second->orphan_seq) oldest = it; }
        if (n <= MAX_ORPHANS) break;
        if (c->stream) { set_device(c); HIP_CHECK(hipStreamSynchronize(c->stream)); }
        plan_free(c, oldest->second);
        c->plans.erase(oldest);
    }
}

// Everything the planner reads goes into the hash: for every node AND leaf the tensor's address and its whole descriptor up to (not including)
// the name - type, ne, nb, op, op_params, flags, the src pointers, view_src / view_offs, data (tensors are zero-filled on creation, so the
// padding bytes are defined). A source is either a node or a leaf of the same graph, so its shape / type / strides / data are covered too.
// Four interleaved multiply-xor lanes keep this at ~15 us for the 1.3 k-node Temporal graph.
static uint64_t graph_hash(const ggml_cgraph * g) {
    constexpr size_t NW = offsetof(ggml_tensor, name) / 8;
    static_assert(offsetof(ggml_tensor, name) % 32 == 0, "tensor descriptor is hashed in 4 lanes of 8-byte words");
    uint64_t h[4] = { 0xcbf29ce484222325ull ^ (uint64_t) g->n_nodes, 0x9e3779b97f4a7c15ull ^ (uint64_t) g->n_leafs, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull };
    auto mix = [&](const ggml_tensor * t) {
        uint64_t w[NW];
        memcpy(w, t, NW * 8);
        w[offsetof(ggml_tensor, buffer) / 8] = 0;   // the buffer OBJECT is not read by the planner (data addresses are): a re-allocated scratch buffer keeps the hash
        h[0] = (h[0] ^ (uint64_t) (uintptr_t) t) * 0x100000001b3ull;
        for (size_t i = 0; i < NW; i += 4) {
            h[0] = (h[0] ^ w[i]) * 0x100000001b3ull; h[1] = (h[1] ^ w[i + 1]) * 0x100000001b3ull;
            h[2] = (h[2] ^ w[i + 2]) * 0x100000001b3ull; h[3] = (h[3] ^ w[i + 3]) * 0x100000001b3ull;
        }
    };
    for (int i = 0; i < g->n_nodes; i++) mix(g->nodes[i]);
    for (int i = 0; i < g->n_leafs; i++) mix(g->leafs[i]);
    uint64_t r = h[0];
    for (int k = 1; k < 4; k++) r = (r ^ (h[k] >> 29) ^ h[k]) * 0x100000001b3ull;
    return r;
}

// ---- graph analysis helpers --------------------------------------------------------------------------
struct analysis {
    const ggml_cgraph * g;
    std::unordered_map<const ggml_tensor *, int> index;          // node -> position
    std::unordered_map<const ggml_tensor *, int> uses;           // tensor -> number of consuming nodes
    std::unordered_map<const ggml_tensor *, int> last_consumer;  // tensor -> position of its (last) consumer
    std::vector<char> skip;
};

static void analyse(analysis & an, const ggml_cgraph * g) {
    an.g = g;
    an.skip.assign((size_t) g->n_nodes, 0);
    for (int i = 0; i < g->n_nodes; i++) {
        const ggml_tensor * n = g->nodes[i];
        an.index[n] = i;
        for (int s = 0; s < GGML_MAX_SRC; s++) {
            const ggml_tensor * src = n->src[s];
            if (!src || src == n) continue;
            bool dup = false;
            for (int s2 = 0; s2 < s; s2++) if (n->src[s2] == src) dup = true;
            if (dup) continue;
            an.uses[src]++;
            an.last_consumer[src] = i;
        }
    }
}
static int uses_of(const analysis & an, const ggml_tensor * t) { auto it = an.uses.find(t); return it == an.uses.end() ? 0 : it->second; }
static int pos_of(const analysis & an, const ggml_tensor * t) { auto it = an.index.find(t); return it == an.index.end() ? -1 : it->second; }
static const ggml_tensor * sole_consumer(const analysis & an, const ggml_tensor * t) {
    if (uses_of(an, t) != 1) return nullptr;
    return an.g->nodes[an.last_consumer.at(t)];
}

static bool is_layout_op(enum ggml_op op) { return op == GGML_OP_VIEW || op == GGML_OP_RESHAPE || op == GGML_OP_PERMUTE || op == GGML_OP_TRANSPOSE; }
static bool is_view_op(enum ggml_op op) { return is_layout_op(op) || op == GGML_OP_NONE; }
static bool is_f32_vec(const ggml_tensor * t, int64_t n) {
    return t->type == GGML_TYPE_F32 && ggml_nelements(t) == n && ggml_is_contiguous(t);
}
static bool dense_rows(const ggml_tensor * w) {
    return w->nb[0] == ggml_type_size(w->type) && w->nb[1] == ggml_row_size(w->type, w->ne[0]) && w->ne[2] == 1 && w->ne[3] == 1;
}

// pointer from which nelements(t) values can be read in t's logical order, looking through layout-only
// nodes and plain dense copies (cont of an already contiguous tensor); NULL when t is not contiguous
static const char * resolve_dense(const ggml_tensor * t) {
    if (!t->data || !ggml_is_contiguous(t)) return nullptr;
    const ggml_tensor * cur = t;
    int64_t delta = 0;
    while (is_layout_op(cur->op)) {
        const ggml_tensor * s = cur->src[0];
        if (!s->data) return nullptr;
        delta += (const char *) cur->data - (const char *) s->data;
        cur = s;
    }
    // cur owns the storage; t's contents are the contiguous byte range cur->data + delta
    if ((cur->op == GGML_OP_CONT || cur->op == GGML_OP_DUP) && cur->src[0]->type == cur->type && ggml_is_contiguous(cur) &&
        ggml_is_contiguous(cur->src[0]) && ggml_nelements(cur->src[0]) == ggml_nelements(cur)) {
        const char * base = resolve_dense(cur->src[0]);   // same bytes, one copy earlier
        if (base) return base + delta;
    }
    return (const char *) cur->data + delta;
}

// Strided view of a tensor's elements in the storage of the earliest tensor that still holds the same values:
// walks through layout-only nodes and through cont/dup copies (mapping strides across the copy). On return element
// (i0,i1,i2,i3) of `t` lives at base + sum i_k * nb[k].
struct sview { const char * base; int64_t ne[4]; int64_t nb[4]; };

static bool strided_resolve(const ggml_tensor * t, sview & sv) {
    if (!t->data) return false;
    sv.base = (const char *) t->data;
    for (int i = 0; i < 4; i++) { sv.ne[i] = t->ne[i]; sv.nb[i] = (int64_t) t->nb[i]; }
    const int64_t es = (int64_t) ggml_type_size(t->type);
    const ggml_tensor * cur = t;
    for (int guard = 0; guard < 8; guard++) {
        while (is_layout_op(cur->op)) cur = cur->src[0];
        if (!(cur->op == GGML_OP_CONT || cur->op == GGML_OP_DUP) || cur->src[0]->type != cur->type || !ggml_is_contiguous(cur) || !cur->data || !cur->src[0]->data) break;
        const ggml_tensor * src = cur->src[0];
        // position of our base inside the dense copy -> logical coordinates of the copy
        int64_t eo = (sv.base - (const char *) cur->data) / es;
        if (eo < 0 || eo >= ggml_nelements(cur)) break;
        int64_t P[5] = { 1, cur->ne[0], cur->ne[0] * cur->ne[1], cur->ne[0] * cur->ne[1] * cur->ne[2], ggml_nelements(cur) };
        int64_t c[4];
        for (int j = 3; j >= 0; j--) { c[j] = eo / P[j]; eo -= c[j] * P[j]; }
        int64_t nb2[4];
        bool ok = true;
        for (int k = 0; k < 4 && ok; k++) {
            nb2[k] = 0;
            if (sv.ne[k] <= 1) continue;
            if (sv.nb[k] % es != 0) { ok = false; break; }
            const int64_t E = sv.nb[k] / es;
            int j = 3;
            while (j > 0 && (P[j] > E || E % P[j] != 0)) j--;
            const int64_t m = E / P[j];
            if (c[j] + m * (sv.ne[k] - 1) >= cur->ne[j]) { ok = false; break; }   // the dim must stay inside one dim of the copy
            nb2[k] = m * (int64_t) src->nb[j];
        }
        if (!ok) break;
        sv.base = (const char *) src->data + c[0] * (int64_t) src->nb[0] + c[1] * (int64_t) src->nb[1] + c[2] * (int64_t) src->nb[2] + c[3] * (int64_t) src->nb[3];
        for (int k = 0; k < 4; k++) sv.nb[k] = nb2[k];
        cur = src;
    }
    return true;
}

// ---- emission ------------------------------------------------------------------------------------------
struct emitter {
    hip_ctx * c;
    plan_t * p;
    void * ws(size_t n) {
        size_t actual = 0;
        void * w = pool_alloc(c, n, &actual);
        GGML_ASSERT(w);
        p->workspaces.push_back({ w, actual });
        return w;
    }
    void push(step_fn f) { p->steps.push_back(pstep(std::move(f))); }
    // Codec convolutions without an im2col launch (match_conv): the output tensor of a conv / transposed-conv group -> a slot its launch reads when it runs.
    // A later conv whose input that tensor is claims the slot (fills it in): the producing launch then also writes the consumer's F16 im2col panel
    // (conv_scatter, hip_common.h), and the consumer starts from the panel.
    std::map<const ggml_tensor *, conv_scatter *> scatter_of;
    conv_scatter * scatter_slot(const ggml_tensor * out) { p->scatter_slots.emplace_back(new conv_scatter()); memset(p->scatter_slots.back().get(), 0, sizeof(conv_scatter)); scatter_of[out] = p->scatter_slots.back().get(); return scatter_of[out]; }
};

static bool is_qblock(enum ggml_type t) { return t == GGML_TYPE_Q4_K || t == GGML_TYPE_Q8_0 || t == GGML_TYPE_Q4_0; }
// BF16 / F16 weights against 2..64 activation rows: the f64-MFMA mat-mul (k_mm_f_batched). MI355X_MMF=0 sends them back to the generic product (the A/B of DESIGN.md 23)
// MI355X_MMF=2 makes the float-accumulating mat-mul (k_mm_f32acc_batched) the starting mode of every fresh handle
static int mmf_env() { static const int v = [] { const char * e = getenv("MI355X_MMF"); return e ? atoi(e) : 1; }(); return v; }
static bool float_batched_ok(const ggml_tensor * w, int64_t T, bool float_acc) {
    if (mmf_env() == 0 || !w->data || (uintptr_t) w->data % 16 != 0 || w->nb[1] % 16 != 0) return false;
    return float_acc ? k_mm_f32acc_batched_supported(w->type, w->ne[0], w->ne[1], T) : k_mm_f_batched_supported(w->type, w->ne[0], w->ne[1], T);
}
// its row converters read the activation rows (and alpha) as float4
static bool aligned16(const void * p) { return p != nullptr && (uintptr_t) p % 16 == 0; }

static bool fill_matvec_base(mv_args & a, const ggml_tensor * mm) {
    const ggml_tensor * w = mm->src[0], * b = mm->src[1];
    if (!dense_rows(w) || !k_matvec_supported(w->type, w->ne[0], w->ne[1])) return false;
    if (b->type != GGML_TYPE_F32 || b->ne[2] != 1 || b->ne[3] != 1 || b->ne[1] < 1) return false;
    if (b->ne[1] > (is_qblock(w->type) ? 1 : MV_MAX_COLS)) return false;
    if (b->nb[0] != 4 || mm->nb[0] != 4) return false;
    memset(&a, 0, sizeof(a));
    a.ncols = (int) b->ne[1];
    a.x_cs = (int64_t) b->nb[1] / 4;
    a.y_cs = (int64_t) mm->nb[1] / 4;
    a.wtype = w->type;
    a.w = (const char *) w->data;
    a.row_bytes = (int64_t) w->nb[1];
    a.K = w->ne[0];
    a.M = w->ne[1];
    a.prologue = MV_PLAIN;
    a.y = (float *) mm->data;
    return true;
}

static void emit_generic(emitter & em, ggml_tensor * n) {
    const tdesc d = make_tdesc(n);
    switch (n->op) {
        case GGML_OP_NONE: case GGML_OP_VIEW: case GGML_OP_RESHAPE: case GGML_OP_PERMUTE: case GGML_OP_TRANSPOSE: return;
        case GGML_OP_ADD: case GGML_OP_SUB: case GGML_OP_MUL: case GGML_OP_DIV: {
            const tdesc a = make_tdesc(n->src[0]), b = make_tdesc(n->src[1]); const int op = n->op;
            em.push([=](hipStream_t s) { k_binary(s, op, d, a, b); });
        } return;
        case GGML_OP_UNARY: {
            const tdesc a = make_tdesc(n->src[0]); const int uop = n->op_params[0];
            em.push([=](hipStream_t s) { k_unary(s, uop, d, a); });
        } return;
        case GGML_OP_SCALE: {
            const tdesc a = make_tdesc(n->src[0]); const float sc = ggml_get_op_params_f32(n, 0), bi = ggml_get_op_params_f32(n, 1);
            em.push([=](hipStream_t s) { k_scale(s, d, a, sc, bi); });
        } return;
        case GGML_OP_CLAMP: {
            const tdesc a = make_tdesc(n->src[0]); const float mn = ggml_get_op_params_f32(n, 0), mx = ggml_get_op_params_f32(n, 1);
            em.push([=](hipStream_t s) { k_clamp(s, d, a, mn, mx); });
        } return;
        case GGML_OP_SUM: { const tdesc a = make_tdesc(n->src[0]); em.push([=](hipStream_t s) { k_sum_all(s, d, a); }); } return;
        case GGML_OP_SUM_ROWS: { const tdesc a = make_tdesc(n->src[0]); em.push([=](hipStream_t s) { k_sum_rows(s, d, a); }); } return;
        case GGML_OP_ARGMAX: { const tdesc a = make_tdesc(n->src[0]); em.push([=](hipStream_t s) { k_argmax(s, d, a); }); } return;
        case GGML_OP_ARGSORT: case GGML_OP_TOP_K: {
            const tdesc a = make_tdesc(n->src[0]); const int desc = n->op_params[0] == GGML_SORT_ORDER_DESC;
            em.push([=](hipStream_t s) { k_argsort(s, d, a, desc); });
        } return;
        case GGML_OP_ARANGE: {
            const float st = ggml_get_op_params_f32(n, 0), step = ggml_get_op_params_f32(n, 2);
            em.push([=](hipStream_t s) { k_arange(s, d, st, step); });
        } return;
        case GGML_OP_REPEAT: { const tdesc a = make_tdesc(n->src[0]); em.push([=](hipStream_t s) { k_repeat(s, d, a); }); } return;
        case GGML_OP_PAD: { const tdesc a = make_tdesc(n->src[0]); em.push([=](hipStream_t s) { k_pad(s, d, a); }); } return;
        case GGML_OP_CONCAT: {
            const tdesc a = make_tdesc(n->src[0]), b = make_tdesc(n->src[1]); const int dim = n->op_params[0];
            em.push([=](hipStream_t s) { k_concat(s, d, a, b, dim); });
        } return;
        case GGML_OP_NORM: case GGML_OP_RMS_NORM: {
            const tdesc a = make_tdesc(n->src[0]); const float eps = ggml_get_op_params_f32(n, 0); const int rms = n->op == GGML_OP_RMS_NORM;
            em.push([=](hipStream_t s) { k_norm(s, d, a, eps, rms); });
        } return;
        case GGML_OP_SOFT_MAX: {
            const tdesc a = make_tdesc(n->src[0]); const int has_mask = n->src[1] != NULL;
            const tdesc m = has_mask ? make_tdesc(n->src[1]) : a; const float sc = ggml_get_op_params_f32(n, 0);
            GGML_ASSERT(ggml_get_op_params_f32(n, 1) == 0.0f && "ALiBi (max_bias) is not used by moshi.cpp");
            em.push([=](hipStream_t s) { k_soft_max(s, d, a, m, has_mask, sc); });
        } return;
        case GGML_OP_CPY: case GGML_OP_CONT: case GGML_OP_DUP: {
            const tdesc a = make_tdesc(n->src[0]);
            em.push([=](hipStream_t s) { k_cpy(s, d, a); });
        } return;
        case GGML_OP_GET_ROWS: {
            const tdesc a = make_tdesc(n->src[0]), idx = make_tdesc(n->src[1]);
            em.push([=](hipStream_t s) { k_get_rows(s, d, a, idx); });
        } return;
        case GGML_OP_SET_ROWS: {
            const tdesc src = make_tdesc(n->src[0]), idx = make_tdesc(n->src[1]);
            em.push([=](hipStream_t s) { k_set_rows(s, d, src, idx); });
        } return;
        case GGML_OP_IM2COL: {
            const tdesc x = make_tdesc(n->src[1]); const int64_t K = n->src[0]->ne[0];
            const int s0 = n->op_params[0], p0 = n->op_params[2], d0 = n->op_params[4];
            em.push([=](hipStream_t s) { k_im2col(s, d, x, K, s0, p0, d0); });
        } return;
        case GGML_OP_CONV_TRANSPOSE_1D: {
            const tdesc w = make_tdesc(n->src[0]), x = make_tdesc(n->src[1]); const int s0 = n->op_params[0];
            void * ws = em.ws(k_conv_transpose_1d_ws_size(n->src[0], n->src[1]));
            em.push([=](hipStream_t s) { k_conv_transpose_1d(s, d, w, x, s0, ws); });
        } return;
        case GGML_OP_TIMESTEP_EMBEDDING: {
            const tdesc ts = make_tdesc(n->src[0]); const int dim = n->op_params[0], mp = n->op_params[1];
            em.push([=](hipStream_t s) { k_timestep_embedding(s, d, ts, dim, mp); });
        } return;
        case GGML_OP_MUL_MAT: {
            mv_args mv;
            if (!(em.c->flags & 1) && fill_matvec_base(mv, n)) {
                mv.x = (const float *) n->src[1]->data;
                em.push([=](hipStream_t s) { k_matvec(s, mv); });
                return;
            }
            {   // several activation rows against Q4_K weights (batched prompt prefill): int8 MFMA tiles
                const ggml_tensor * w0 = n->src[0], * x1 = n->src[1];
                const int64_t Tn = ggml_nelements(x1) / x1->ne[0];
                static const bool no_batched = getenv("MI355X_NO_BATCHED_MM") != nullptr;
                if (!no_batched && x1->type == GGML_TYPE_F32 && ggml_is_contiguous(x1) && ggml_is_contiguous(n) && ggml_is_contiguous(w0) && w0->ne[2] == 1 && w0->ne[3] == 1 &&
                    k_mm_q4k_batched_supported(w0->type, w0->ne[0], w0->ne[1], Tn)) {
                    const char * wp = (const char *) w0->data; const int64_t rb = (int64_t) w0->nb[1], K = w0->ne[0], M = w0->ne[1];
                    const float * xp = (const float *) x1->data; float * yp = (float *) n->data;
                    void * ws = em.ws(k_mm_q4k_batched_ws_size(K, Tn));
                    const int wt = (int) w0->type;
                    em.push([=](hipStream_t s) { k_mm_q4k_batched(s, wt, wp, rb, K, M, Tn, xp, K, ws, yp, M, nullptr, 0); });
                    return;
                }
                // ... against BF16 / F16 weights: f64 MFMA tiles
                if (!no_batched && x1->type == GGML_TYPE_F32 && ggml_is_contiguous(x1) && n->type == GGML_TYPE_F32 && ggml_is_contiguous(n) && ggml_is_contiguous(w0) &&
                    w0->ne[2] == 1 && w0->ne[3] == 1 && aligned16(x1->data) && float_batched_ok(w0, Tn, em.c->float_acc != 0)) {
                    const char * wp = (const char *) w0->data; const int64_t rb = (int64_t) w0->nb[1], K = w0->ne[0], M = w0->ne[1];
                    const float * xp = (const float *) x1->data; float * yp = (float *) n->data;
                    void * ws = em.ws(k_mm_f_batched_ws_size(K, Tn));
                    const int wt = (int) w0->type;
                    if (em.c->float_acc) { em.push([=](hipStream_t s) { k_mm_f32acc_batched(s, wt, wp, rb, K, M, Tn, xp, K, ws, yp, M, nullptr, 0); }); em.p->n_float_acc_mms++; }
                    else { em.push([=](hipStream_t s) { k_mm_f_batched(s, wt, wp, rb, K, M, Tn, xp, K, ws, yp, M, nullptr, 0); }); em.p->n_float_batched_mms++; }
                    return;
                }
            }
            const tdesc a = make_tdesc(n->src[0]), b = make_tdesc(n->src[1]);
            void * w = em.ws(k_mul_mat_ws_size(n->src[0], n->src[1]));
            em.push([=](hipStream_t s) { k_mul_mat(s, d, a, b, w); });
        } return;
        default:
            GGML_ABORT("mi355x backend: unsupported op %s (node %s)", ggml_op_name(n->op), n->name);
    }
}

// ---- fusion matchers --------------------------------------------------------------------------------------
// what every matcher returns: the nodes one launch replaces and the position at which that launch is emitted (embedding sums: where they matched)
struct group { int emit_pos = -1; std::vector<int> members; };

// A. mat-vec with fused activation prologue and residual epilogue. Returns the position at which the
//    fused kernel must be emitted (the last node of the group), or -1.
struct mv_group : group { mv_args a; };
static bool match_embed_term(const analysis & an, const ggml_tensor * e, embed_src & out, std::vector<int> & members, int64_t B = 1);

static bool writes_through_alias(const ggml_tensor * n) {
    return n->view_src != NULL && !is_view_op(n->op);
}

static bool match_matvec(const analysis & an, int pos, mv_group & grp) {
    ggml_tensor * mm = an.g->nodes[pos];
    if (mm->op != GGML_OP_MUL_MAT || !fill_matvec_base(grp.a, mm)) return false;
    mv_args & a = grp.a;
    const ggml_tensor * b = mm->src[1];
    const int64_t K = a.K;
    grp.members.clear();
    grp.members.push_back(pos);
    grp.emit_pos = pos;
    bool have_x = false;
    // per-step weight selection wraps the activation in a whole-tensor view (transformer.h:85-91): look through it
    while ((b->op == GGML_OP_VIEW || b->op == GGML_OP_RESHAPE) && uses_of(an, b) == 1 && b->src[0]->data == b->data &&
           ggml_nelements(b->src[0]) == ggml_nelements(b) && ggml_is_contiguous(b->src[0])) b = b->src[0];

    // prologue 1: b = alpha * rms_norm(x), private to this mat-vec - or shared with exactly one cpy(b -> contiguous F32 tensor) issued right before the
    // mat-vec (the Temporal head: out_norm feeds text_linear and is kept as the `transformer_out` state, lm.h:434): workgroup 0 writes the copy
    const ggml_tensor * side_cpy = nullptr;
    if (a.ncols == 1 && b->op == GGML_OP_MUL && uses_of(an, b) == 2 && pos > 0 && is_qblock(mm->src[0]->type)) {
        const ggml_tensor * cp = an.g->nodes[pos - 1];
        if (cp->op == GGML_OP_CPY && cp->src[0] == b && cp->type == GGML_TYPE_F32 && ggml_is_contiguous(cp) && ggml_nelements(cp) == K && cp->data &&
            !an.skip[(size_t) (pos - 1)]) side_cpy = cp;
    }
    if (a.ncols == 1 && b->op == GGML_OP_MUL && is_f32_vec(b, K) && (uses_of(an, b) == 1 || side_cpy) && (!is_qblock(mm->src[0]->type) || K <= 4096)) {
        const ggml_tensor * al = b->src[0], * nr = b->src[1];
        if (nr->op != GGML_OP_RMS_NORM) std::swap(al, nr);
        if (nr->op == GGML_OP_RMS_NORM && uses_of(an, nr) == 1 && is_f32_vec(al, K) && is_f32_vec(nr->src[0], K)) {
            a.prologue = MV_RMSNORM;
            a.x = (const float *) nr->src[0]->data;
            a.alpha = (const float *) al->data;
            a.eps = ggml_get_op_params_f32(nr, 0);
            grp.members.push_back(pos_of(an, b)); grp.members.push_back(pos_of(an, nr));
            if (side_cpy) { a.x_out = (float *) side_cpy->data; grp.members.push_back(pos - 1); }
            have_x = true;
        }
    }
    // prologue 1b: b = norm(x) * w (+ bias) (torch_nn_layer_norm, torch.h:49-60), any column count
    if (!have_x && !is_qblock(mm->src[0]->type) && uses_of(an, b) == 1 && (b->op == GGML_OP_ADD || b->op == GGML_OP_MUL)) {
        const ggml_tensor * mulw = b, * bias = nullptr;
        if (b->op == GGML_OP_ADD && b->src[0]->op == GGML_OP_MUL && uses_of(an, b->src[0]) == 1) { mulw = b->src[0]; bias = b->src[1]; }
        if (mulw->op == GGML_OP_MUL && mulw->src[0]->op == GGML_OP_NORM && uses_of(an, mulw->src[0]) == 1) {
            const ggml_tensor * nr = mulw->src[0], * wgt = mulw->src[1], * xin = nr->src[0];
            if (is_f32_vec(wgt, K) && (!bias || is_f32_vec(bias, K)) && xin->type == GGML_TYPE_F32 && xin->ne[0] == K && xin->ne[1] == a.ncols &&
                xin->nb[0] == 4 && ggml_nelements(xin) == K * a.ncols && ggml_are_same_shape(b, xin)) {
                a.prologue = MV_LAYERNORM;
                a.x = (const float *) xin->data;
                a.x_cs = (int64_t) xin->nb[1] / 4;
                a.alpha = (const float *) wgt->data;
                a.beta = bias ? (const float *) bias->data : nullptr;
                a.eps = ggml_get_op_params_f32(nr, 0);
                grp.members.push_back(pos_of(an, nr)); grp.members.push_back(pos_of(an, mulw));
                if (bias) grp.members.push_back(pos_of(an, b));
                have_x = true;
            }
        }
    }
    // prologue 1c: b = gelu(h)
    if (!have_x && !is_qblock(mm->src[0]->type) && b->op == GGML_OP_UNARY && b->op_params[0] == GGML_UNARY_OP_GELU && uses_of(an, b) == 1 &&
        !an.skip[(size_t) pos_of(an, b)]) {   // (already produced by the previous mat-vec's epilogue otherwise)
        const ggml_tensor * hin = b->src[0];
        if (hin->type == GGML_TYPE_F32 && hin->nb[0] == 4 && ggml_are_same_shape(hin, b) && hin->ne[2] == 1 && hin->ne[3] == 1) {
            a.prologue = MV_GELU;
            a.x = (const float *) hin->data;
            a.x_cs = (int64_t) hin->nb[1] / 4;
            grp.members.push_back(pos_of(an, b));
            have_x = true;
        }
    }
    // prologue 2: b = silu(left(h)) * right(h)
    if (!have_x && a.ncols == 1 && b->op == GGML_OP_MUL && uses_of(an, b) == 1 && ggml_nelements(b) == K) {
        const ggml_tensor * sl = b->src[0], * r = b->src[1];
        if (sl->op == GGML_OP_UNARY && sl->op_params[0] == GGML_UNARY_OP_SILU && uses_of(an, sl) == 1 &&
            sl->src[0]->op == GGML_OP_VIEW && r->op == GGML_OP_VIEW && uses_of(an, sl->src[0]) == 1 && uses_of(an, r) == 1) {
            const ggml_tensor * l = sl->src[0];
            const ggml_tensor * h = l->src[0];
            if (r->src[0] == h && is_f32_vec(h, 2 * K) && l->data == h->data && (const char *) r->data == (const char *) h->data + K * 4 &&
                ggml_is_contiguous(l) && ggml_is_contiguous(r)) {
                a.prologue = MV_GATE_SILU;
                a.x = (const float *) h->data;
                grp.members.push_back(pos_of(an, b)); grp.members.push_back(pos_of(an, sl));
                have_x = true;
            }
        }
    }
    if (!have_x) {   // plain activation: address it through the mat-vec's own operand (a looked-through view may be shaped differently)
        a.x = (const float *) mm->src[1]->data;
        a.x_cs = (int64_t) mm->src[1]->nb[1] / 4;
    }
    // epilogue 0: gelu(W x) (the activation is evaluated once per output element here, not once per consuming workgroup)
    {
        const ggml_tensor * g = sole_consumer(an, mm);
        if (g && g->op == GGML_OP_UNARY && g->op_params[0] == GGML_UNARY_OP_GELU && !is_qblock(mm->src[0]->type) && g->view_src == NULL &&
            ggml_are_same_shape(g, mm) && g->nb[0] == 4 && g->type == GGML_TYPE_F32) {
            a.out_act = 1;
            a.y = (float *) g->data;
            a.y_cs = (int64_t) g->nb[1] / 4;
            grp.members.push_back(pos_of(an, g));
            grp.emit_pos = pos_of(an, g);
            return true;
        }
    }
    // epilogue: (optional per-row layer_scale, then) the only consumer adds a same-shaped F32 tensor
    const ggml_tensor * cons = sole_consumer(an, mm);
    const ggml_tensor * scaled = nullptr;
    if (cons && cons->op == GGML_OP_MUL && cons->view_src == NULL && cons->src[0] == mm && !is_qblock(mm->src[0]->type) &&
        is_f32_vec(cons->src[1], a.M) && ggml_are_same_shape(cons, mm) && cons->nb[0] == 4) {
        const ggml_tensor * c2 = sole_consumer(an, cons);
        if (c2 && c2->op == GGML_OP_ADD) { scaled = cons; cons = c2; }
    }
    const ggml_tensor * prod = scaled ? scaled : mm;
    if (cons && cons->op == GGML_OP_ADD && cons->view_src == NULL) {
        const ggml_tensor * other = cons->src[0] == prod ? cons->src[1] : cons->src[0];
        const bool shapes = other != prod && other->type == GGML_TYPE_F32 && ggml_are_same_shape(other, mm) && ggml_are_same_shape(cons, mm) &&
                            other->nb[0] == 4 && cons->nb[0] == 4 && cons->type == GGML_TYPE_F32;
        // the addend is one embedding row (moshi_scaled_embedding_chained + cast, lm.h:446-475): gather it in the epilogue
        std::vector<int> emb_members;
        embed_src es;
        const ggml_tensor * term = other;
        bool embed = false;
        if (shapes && !scaled && is_qblock((enum ggml_type) a.wtype) && a.ncols == 1 && uses_of(an, other) == 1) {
            if (term->op == GGML_OP_CPY && term->view_src == NULL && term->src[0]->type == GGML_TYPE_F32 && ggml_are_same_shape(term->src[0], term) && uses_of(an, term->src[0]) == 1) {
                emb_members.push_back(pos_of(an, term));
                term = term->src[0];
            }
            embed = (term->op == GGML_OP_GET_ROWS || term->op == GGML_OP_MUL) && term->ne[1] == 1 && match_embed_term(an, term, es, emb_members);
            for (int m : emb_members) if (m < 0 || an.skip[(size_t) m]) embed = false;
        }
        if (shapes && embed) for (int i = pos + 1; i < pos_of(an, cons); i++) if (writes_through_alias(an.g->nodes[i])) embed = false;
        if (shapes && embed) {
            const int cpos = pos_of(an, cons);
            a.res_embed = es;
            a.y = (float *) cons->data;
            a.y_cs = (int64_t) cons->nb[1] / 4;
            for (int m : emb_members) grp.members.push_back(m);
            grp.members.push_back(cpos);
            grp.emit_pos = cpos;
        } else if (shapes) {
            const int cpos = pos_of(an, cons);
            bool hazard = false;
            for (int i = pos + 1; i < cpos; i++) if (writes_through_alias(an.g->nodes[i])) hazard = true;
            if (!hazard) {
                a.residual = (const float *) other->data;
                a.r_cs = (int64_t) other->nb[1] / 4;
                a.y = (float *) cons->data;
                a.y_cs = (int64_t) cons->nb[1] / 4;
                if (scaled) { a.out_scale = (const float *) scaled->src[1]->data; grp.members.push_back(pos_of(an, scaled)); }
                grp.members.push_back(cpos);
                grp.emit_pos = cpos;
            }
        }
    }
    return true;
}

// A''. LayerNorm with weight (and bias) over one row that no mat-vec prologue took (tts: norm_cross in front of the cross-attention's row-view projection):
//      ggml_norm -> ggml_mul(., w) -> [ggml_add(., b)] as one launch with the three launches' float operations, matched at the norm
struct norm_affine_group : group { tdesc x; float eps; int rms; const float * w, * b; float * out; };
static bool match_norm_affine(const analysis & an, int pos, norm_affine_group & grp) {
    const ggml_tensor * nn = an.g->nodes[pos];
    if ((nn->op != GGML_OP_NORM && nn->op != GGML_OP_RMS_NORM) || nn->type != GGML_TYPE_F32 || uses_of(an, nn) != 1) return false;
    if (nn->src[0]->type != GGML_TYPE_F32 || nn->src[0]->nb[0] != 4) return false;
    // one row, or the B contiguous rows of a B-column LM activation [dim, 1, B] under the same [dim] weight and bias (norm_cross of B-column tts
    // steps), one workgroup per row. Only that layout and LayerNorm: every other multi-row norm keeps the plan it had.
    const int64_t n_rows = ggml_nelements(nn) / nn->ne[0];
    if (n_rows != 1 && (nn->op != GGML_OP_NORM || nn->ne[1] != 1 || nn->ne[2] != n_rows || n_rows > 16 || !ggml_is_contiguous(nn) || !ggml_is_contiguous(nn->src[0]))) return false;
    const ggml_tensor * ml = sole_consumer(an, nn);
    if (!ml || ml->op != GGML_OP_MUL || ml->view_src || pos_of(an, ml) < 0 || an.skip[(size_t) pos_of(an, ml)] || !ggml_are_same_shape(ml, nn)) return false;
    const ggml_tensor * wv = ml->src[0] == nn ? ml->src[1] : ml->src[0];
    if (wv == nn || wv->type != GGML_TYPE_F32 || !ggml_is_contiguous(wv) || ggml_nelements(wv) != nn->ne[0] || !wv->data || !ggml_is_contiguous(ml)) return false;
    grp.members = { pos, pos_of(an, ml) };
    const ggml_tensor * last = ml;
    grp.b = nullptr;
    const ggml_tensor * ad = uses_of(an, ml) == 1 ? sole_consumer(an, ml) : nullptr;
    if (ad && ad->op == GGML_OP_ADD && !ad->view_src && pos_of(an, ad) >= 0 && !an.skip[(size_t) pos_of(an, ad)] && ggml_is_contiguous(ad)) {
        const ggml_tensor * bv = ad->src[0] == ml ? ad->src[1] : ad->src[0];
        if (bv != ml && bv->type == GGML_TYPE_F32 && ggml_is_contiguous(bv) && ggml_nelements(bv) == nn->ne[0] && bv->data && bv->op == GGML_OP_NONE && ad->src[0] == ml && ggml_are_same_shape(ad, nn)) {
            grp.b = (const float *) bv->data; last = ad; grp.members.push_back(pos_of(an, ad));
        }
    }
    // (the weight must be the second factor or the first: the product is the same float either way; the bias must be the second summand: v + b)
    grp.x = make_tdesc(nn->src[0]); grp.eps = ggml_get_op_params_f32(nn, 0); grp.rms = nn->op == GGML_OP_RMS_NORM;
    grp.w = (const float *) wv->data; grp.out = (float *) last->data;
    grp.emit_pos = pos_of(an, last);
    return true;
}

// B. the self-attention block of one Temporal / Depth layer (moshi_hot.cpp), matched at its soft_max. One block walk, four forms:
//      single column  q / k / v [D, T, H], whole rings [D, C, H], T <= 64 new rows, output a dense [D, H, T] of its own (match_attention; T > 4 is batched prompt prefill)
//      ring column    the same over [D, C, H] views of ONE column of [D, C, H, B] rings (slot prefill): `column`, a job of a k_attn_blocks launch pair or, as a run of
//                     ring-ordered one-row groups, of a k_attn_rows launch; its output may be a copy into the block's row range of a wider [D, H, T] tensor
//      lockstep       one row of B > 1 columns (moshi_hot_create_streams): q / k / v [D, 1, H, B], rings [D, C, H, B] written at one shared slot, one shared mask row and
//                     RoPE phase, output [D, H, 1, B] - one launch of B x H workgroups, k_attn_streams (match_attention_streams)
//      slots          the same with every column at its own position (moshi_hot_create_slots): a mask [C, 1, 1, B] (one contiguous row per stream), an index [1, 1, B]
//                     (one ring slot per stream), RoPE halves [D/2, 1, 1, B] (one timestep-table row per stream) - the same launch with per-stream strides
//      decoder slots  T = 2 rows of B > 1 columns, every column at its own position (moshi_hot_create_codec_slots): mask [C, T, 1, B], index [T, 1, B], RoPE halves
//                     [D/2, T, 1, B] - one launch of H x T x B workgroups, k_attn_codec_slots (match_attention_codec_slots; the codec transformers' shape only)
//      Refused today: several rows of several columns at once in any other shape, and a copy into rows from anything but a ring column.
struct attn_group : group { attn_args a; const ggml_tensor * mask_node; int B = 1; attn_streams_args sa;   // B > 1: match_attention_streams
                          bool column = false; };   // the rings are one column of [D, C, H, B] rings (slot prefill): the group is a job of a k_attn_blocks launch pair

// rotated = concat(sub(mul(r, rotr), mul(i, roti)), add(mul(r, roti), mul(i, rotr))); returns the un-rotated source
static bool match_rope(const ggml_tensor * rotated, const ggml_tensor ** src_out, const ggml_tensor ** rotr_out, const ggml_tensor ** roti_out) {
    if (rotated->op != GGML_OP_CONCAT || rotated->op_params[0] != 0) return false;
    const ggml_tensor * re = rotated->src[0], * im = rotated->src[1];
    if (re->op != GGML_OP_SUB || im->op != GGML_OP_ADD) return false;
    const ggml_tensor * m0 = re->src[0], * m1 = re->src[1], * m2 = im->src[0], * m3 = im->src[1];
    if (m0->op != GGML_OP_MUL || m1->op != GGML_OP_MUL || m2->op != GGML_OP_MUL || m3->op != GGML_OP_MUL) return false;
    const ggml_tensor * xr = m0->src[0], * rotr = m0->src[1], * xi = m1->src[0], * roti = m1->src[1];
    if (m2->src[0] != xr || m2->src[1] != roti || m3->src[0] != xi || m3->src[1] != rotr) return false;
    // xr / xi = reshape(view(Z, half 0 / 1)), Z = cont(permute(reshape(cont(src), 2, D/2, T, BH), 3, 0, 1, 2))
    if (xr->op != GGML_OP_RESHAPE || xi->op != GGML_OP_RESHAPE) return false;
    const ggml_tensor * vr = xr->src[0], * vi = xi->src[0];
    if (vr->op != GGML_OP_VIEW || vi->op != GGML_OP_VIEW || vr->src[0] != vi->src[0]) return false;
    const ggml_tensor * Z = vr->src[0];
    if (Z->op != GGML_OP_CONT || vr->data != Z->data || (const char *) vi->data != (const char *) Z->data + ggml_nbytes(Z) / 2) return false;
    const ggml_tensor * P = Z->src[0];
    if (P->op != GGML_OP_PERMUTE || P->op_params[0] != 3 || P->op_params[1] != 0 || P->op_params[2] != 1 || P->op_params[3] != 2) return false;
    const ggml_tensor * R = P->src[0];
    if (R->op != GGML_OP_RESHAPE || R->ne[0] != 2) return false;
    *src_out = R->src[0];
    *rotr_out = rotr;
    *roti_out = roti;
    return true;
}

// THE CHAIN, from the soft_max at `pos`: x2 = sole consumer of x1 = permute(pv), pv = mul_mat(cont(transpose(vc)), sm), sm = soft_max(kq, mask),
// kq = mul_mat(kc, qo), kc / vc = set_rows(ring, ko / vrow, idx). Guaranteed on return: kq, sm, pv and x1 have one consumer each; the rings are BF16 with
// dense rows, of one shape [D, C, H] in their first three dimensions, written at one shared contiguous I32 index; D fits the kernels' lane layout; the mask
// is contiguous F32 rows of C. What x2 is (cont, or a copy into rows) and every size beyond D, C, H is the caller's to check.
struct attn_chain { const ggml_tensor * sm, * kq, * pv, * kc, * vc, * qo, * ko, * vrow, * x1, * x2, * mask, * idx; };
static bool match_attention_chain(const analysis & an, int pos, attn_chain & c) {
    c.sm = an.g->nodes[pos];
    if (c.sm->op != GGML_OP_SOFT_MAX || !c.sm->src[1]) return false;
    c.kq = c.sm->src[0]; c.mask = c.sm->src[1];
    if (c.kq->op != GGML_OP_MUL_MAT || uses_of(an, c.kq) != 1 || uses_of(an, c.sm) != 1) return false;
    c.kc = c.kq->src[0]; c.qo = c.kq->src[1];
    if (c.kc->op != GGML_OP_SET_ROWS || c.kc->type != GGML_TYPE_BF16) return false;
    c.pv = sole_consumer(an, c.sm);
    if (!c.pv || c.pv->op != GGML_OP_MUL_MAT || c.pv->src[1] != c.sm) return false;
    const ggml_tensor * vt = c.pv->src[0];
    if (vt->op != GGML_OP_CONT || vt->src[0]->op != GGML_OP_TRANSPOSE) return false;
    c.vc = vt->src[0]->src[0];
    if (c.vc->op != GGML_OP_SET_ROWS || c.vc->type != GGML_TYPE_BF16) return false;
    c.x1 = sole_consumer(an, c.pv);
    if (!c.x1 || c.x1->op != GGML_OP_PERMUTE) return false;
    c.x2 = sole_consumer(an, c.x1);
    if (!c.x2) return false;
    const int64_t D = c.kc->ne[0];
    if (c.vc->ne[0] != D || c.vc->ne[1] != c.kc->ne[1] || c.vc->ne[2] != c.kc->ne[2] || c.kc->nb[0] != 2 || c.vc->nb[0] != 2) return false;
    if (D % 8 != 0 || 64 % (D / 8) != 0 || D > 256) return false;
    if (c.mask->type != GGML_TYPE_F32 || c.mask->ne[0] != c.kc->ne[1] || !ggml_is_contiguous(c.mask)) return false;
    c.idx = c.kc->src[1];
    if (c.vc->src[1] != c.idx || c.idx->type != GGML_TYPE_I32 || !ggml_is_contiguous(c.idx)) return false;
    c.ko = c.kc->src[0]; c.vrow = c.vc->src[0];
    return true;
}

// THE ROPE PAIR: q and k un-rotated, or both rotated (match_rope) by the same F32 table halves of D / 2 dense values, roti directly behind rotr.
// rotr == nullptr: no RoPE. How many table rows there are and how they are strided differs by form: the caller's check.
struct rope_pair { const ggml_tensor * qsrc, * ksrc, * rotr, * roti; };
static bool match_rope_pair(const attn_chain & c, rope_pair & r) {
    r = { c.qo, c.ko, nullptr, nullptr };
    if (c.qo->op != GGML_OP_CONCAT) return true;
    const ggml_tensor * rotr2, * roti2;
    const int64_t D = c.kc->ne[0];
    if (!match_rope(c.qo, &r.qsrc, &r.rotr, &r.roti) || !match_rope(c.ko, &r.ksrc, &rotr2, &roti2) || r.rotr != rotr2 || r.roti != roti2) return false;
    return r.rotr->type == GGML_TYPE_F32 && r.rotr->ne[0] == D / 2 && r.rotr->nb[0] == 4 && (const char *) r.roti->data == (const char *) r.rotr->data + D / 2 * 4;
}

// THE INTERIOR: everything reachable from x2 down to the block's inputs - the projections' mul_mats and timestep tables, the mask, the index, the RoPE
// table and leaves (rings, weights) - as graph positions. into_rows: x2 is a cpy into rows of a wider tensor, whose destination is not followed (it leads
// to the previous job). Guaranteed: every member is one of the listed ops and stands at most 200 nodes before the soft_max; the block holds exactly two
// mul_mats, one soft_max and two set_rows; and no interior value is consumed outside the block (x2 is its output): every consumer of a member is a
// member - counted from the members' side (the analysis holds every tensor's number of consuming nodes), so a graph of many blocks is not walked once per block.
static bool collect_attention_interior(const analysis & an, int pos, const attn_chain & c, const rope_pair & r, bool into_rows, std::vector<int> & members) {
    std::vector<const ggml_tensor *> stack = { c.x2 };
    std::unordered_map<const ggml_tensor *, bool> seen;
    int n_mm = 0, n_sm = 0, n_sr = 0;
    const int lo = pos - 200 > 0 ? pos - 200 : 0;
    while (!stack.empty()) {
        const ggml_tensor * t = stack.back(); stack.pop_back();
        if (seen[t]) continue;
        seen[t] = true;
        const int p = pos_of(an, t);
        if (p < 0) continue;                                  // leaf: cache, mask, indices, weights
        if (t == c.mask || t == c.idx || t == r.rotr || t == r.roti) continue;
        if ((const char *) t->data == nullptr) return false;
        // the projection output (and anything before it) is an input of the block, not part of it
        const bool is_input = (t->op == GGML_OP_MUL_MAT && t != c.kq && t != c.pv) || t->op == GGML_OP_TIMESTEP_EMBEDDING;
        if (is_input) continue;
        if (p < lo) return false;                              // wandered out of the layer: refuse
        switch (t->op) {
            case GGML_OP_MUL_MAT: n_mm++; break;
            case GGML_OP_SOFT_MAX: n_sm++; break;
            case GGML_OP_SET_ROWS: n_sr++; break;
            case GGML_OP_VIEW: case GGML_OP_RESHAPE: case GGML_OP_PERMUTE: case GGML_OP_TRANSPOSE: case GGML_OP_CONT:
            case GGML_OP_MUL: case GGML_OP_SUB: case GGML_OP_ADD: case GGML_OP_CONCAT: break;
            case GGML_OP_CPY: if (t != c.x2 || !into_rows) return false; break;
            default: return false;
        }
        members.push_back(p);
        if (t == c.x2 && into_rows) { stack.push_back(t->src[0]); continue; }
        for (int s = 0; s < GGML_MAX_SRC; s++) if (t->src[s]) stack.push_back(t->src[s]);
    }
    if (n_mm != 2 || n_sm != 1 || n_sr != 2) return false;
    std::unordered_map<int, int> consumed;   // member position -> consuming nodes inside the block
    for (int p : members) consumed[p] = 0;
    for (int p : members) {
        const ggml_tensor * n = an.g->nodes[p];
        for (int s = 0; s < GGML_MAX_SRC; s++) {
            const ggml_tensor * t = n->src[s];
            if (!t || t == n) continue;
            bool dup = false;
            for (int s2 = 0; s2 < s; s2++) if (n->src[s2] == t) dup = true;
            if (dup) continue;
            auto it = consumed.find(pos_of(an, t));
            if (it != consumed.end()) it->second++;
        }
    }
    for (auto & kv : consumed) if (an.g->nodes[kv.first] != c.x2 && kv.second != uses_of(an, an.g->nodes[kv.first])) return false;
    return true;
}

// q / k / v as the projection left them: F32 [D, n1, H, n3], their first dimension dense (strided_resolve looks through the layout nodes and copies)
static bool resolve_qkv(const attn_chain & c, const rope_pair & r, int64_t n1, int64_t n3, sview & qs, sview & ks, sview & vs) {
    for (const ggml_tensor * t : { r.qsrc, r.ksrc, c.vrow })
        if (t->type != GGML_TYPE_F32 || t->ne[0] != c.kc->ne[0] || t->ne[1] != n1 || t->ne[2] != c.kc->ne[2] || t->ne[3] != n3) return false;
    return strided_resolve(r.qsrc, qs) && strided_resolve(r.ksrc, ks) && strided_resolve(c.vrow, vs) && qs.nb[0] == 4 && ks.nb[0] == 4 && vs.nb[0] == 4;
}

// THE COMMON ARGUMENTS of every form: bases, head strides, ring strides, H D C, scale, out and its row stride, members and emit position. A mask that is a
// dense copy, made in this graph, of an already dense row is bypassed (the source is read) and named in mask_node: pass_attention drops the copy when
// every consumer bypasses it. T, the row strides of q / k / v and everything per stream are the caller's.
static void fill_attention_group(const analysis & an, const attn_chain & c, const rope_pair & r, const sview & qs, const sview & ks, const sview & vs,
                                 const std::vector<int> & members, attn_group & grp) {
    attn_args & a = grp.a;
    memset(&a, 0, sizeof(a));
    a.q = (const float *) qs.base; a.k = (const float *) ks.base; a.v = (const float *) vs.base;
    a.q_hs = qs.nb[2] / 4; a.k_hs = ks.nb[2] / 4; a.v_hs = vs.nb[2] / 4;
    a.rot = r.rotr ? (const float *) r.rotr->data : nullptr;
    a.mask = (const float *) c.mask->data;
    grp.mask_node = nullptr;
    if (c.mask->op == GGML_OP_CONT && pos_of(an, c.mask) >= 0) {
        const char * base = resolve_dense(c.mask);
        if (base && base != (const char *) c.mask->data) { a.mask = (const float *) base; grp.mask_node = c.mask; }
    }
    a.index = (const int32_t *) c.idx->data;
    a.kcache = (char *) c.kc->data; a.vcache = (char *) c.vc->data;
    a.k_nb1 = (int64_t) c.kc->nb[1]; a.k_nb2 = (int64_t) c.kc->nb[2];
    a.v_nb1 = (int64_t) c.vc->nb[1]; a.v_nb2 = (int64_t) c.vc->nb[2];
    a.H = (int) c.kc->ne[2]; a.D = (int) c.kc->ne[0]; a.C = (int) c.kc->ne[1];
    a.scale = ggml_get_op_params_f32(c.sm, 0);
    a.out = (float *) c.x2->data;
    a.out_ts = c.kc->ne[2] * c.kc->ne[0];
    grp.members = members;
    grp.emit_pos = pos_of(an, c.x2);
}

// the single-column and ring-column forms: T rows of one column
static bool match_attention(const analysis & an, int pos, attn_group & grp) {
    attn_chain c; rope_pair r;
    if (!match_attention_chain(an, pos, c)) return false;
    const ggml_tensor * kc = c.kc, * vc = c.vc, * x2 = c.x2;
    // the block's output: a dense copy of its own, or (slot prefill) a copy into the block's row range of a wider [D, H, T] tensor
    const bool into_rows = x2->op == GGML_OP_CPY && x2->src[0] == c.x1 && x2->type == GGML_TYPE_F32;
    if (x2->op != GGML_OP_CONT && !into_rows) return false;
    // the rings: whole [D, C, H] tensors, or (slot prefill) [D, C, H] views of one column of [D, C, H, B] rings
    const bool column = kc->ne[3] == 1 && kc->view_src && kc->view_src->ne[3] > 1;
    if (column != (vc->ne[3] == 1 && vc->view_src && vc->view_src->ne[3] > 1) || (into_rows && !column)) return false;

    const int64_t D = kc->ne[0], H = kc->ne[2], Tn = c.qo->ne[1];
    if (c.qo->ne[0] != D || Tn < 1 || Tn > 64 || c.qo->ne[2] != H || c.qo->ne[3] != 1) return false;   // B == 1; blocks longer than 4 rows (prompt prefill) run as consecutive launches of 4
    if (c.mask->ne[1] != Tn || ggml_nelements(c.idx) != Tn) return false;
    if (!match_rope_pair(c, r)) return false;
    if (r.rotr && (r.rotr->ne[1] != Tn || (Tn > 1 && (int64_t) r.rotr->nb[1] != D * 4))) return false;   // one table row per block row
    sview qs, ks, vs;
    if (!resolve_qkv(c, r, Tn, 1, qs, ks, vs)) return false;
    for (const sview * v : { &qs, &ks, &vs }) if (v->nb[1] % 4 != 0 || v->nb[2] % 4 != 0) return false;
    if (x2->ne[0] != D || x2->ne[1] != H || x2->ne[2] != Tn || !ggml_is_contiguous(x2)) return false;
    std::vector<int> members;
    if (!collect_attention_interior(an, pos, c, r, into_rows, members)) return false;
    fill_attention_group(an, c, r, qs, ks, vs, members, grp);
    grp.a.T = (int) Tn;
    grp.a.q_ts = qs.nb[1] / 4; grp.a.k_ts = ks.nb[1] / 4; grp.a.v_ts = vs.nb[1] / 4;
    grp.column = column;
    return true;
}

// the lockstep and slots forms: one row of B > 1 columns; what is per stream (mask row, ring slot, RoPE row) gets a stride, what is shared gets 0
static bool match_attention_streams(const analysis & an, int pos, attn_group & grp) {
    attn_chain c; rope_pair r;
    if (!match_attention_chain(an, pos, c) || c.x2->op != GGML_OP_CONT) return false;
    const ggml_tensor * kc = c.kc, * vc = c.vc, * mask = c.mask, * idx = c.idx, * x2 = c.x2;
    const int64_t D = kc->ne[0], C = kc->ne[1], H = kc->ne[2], B = kc->ne[3];
    if (B < 2 || c.qo->ne[0] != D || c.qo->ne[1] != 1 || c.qo->ne[2] != H || c.qo->ne[3] != B || vc->ne[3] != B || mask->ne[1] != 1) return false;
    const bool mask_per_stream = mask->ne[2] == 1 && mask->ne[3] == B && ggml_nelements(mask) == C * B;   // one row per stream (slots)
    if (!mask_per_stream && ggml_nelements(mask) != C) return false;                                      // or one shared row
    const bool index_per_stream = idx->ne[0] == 1 && idx->ne[1] == 1 && idx->ne[2] == B && ggml_nelements(idx) == B;   // one ring slot per stream (slots)
    if (!index_per_stream && ggml_nelements(idx) != 1) return false;                                                    // or one shared slot
    if (!match_rope_pair(c, r)) return false;
    int64_t rot_bs = 0;
    if (r.rotr) {
        const ggml_tensor * rotr = r.rotr, * roti = r.roti;
        if (rotr->ne[1] != 1) return false;
        if (ggml_nelements(rotr) == D / 2) rot_bs = 0;                                                            // one shared RoPE row
        else if (rotr->ne[2] == 1 && rotr->ne[3] == B && roti->type == GGML_TYPE_F32 && ggml_are_same_shape(rotr, roti) && roti->nb[3] == rotr->nb[3] &&
                 (int64_t) rotr->nb[3] == D * 4) rot_bs = D;                                                       // one row of the [D, B] table per stream
        else return false;
    }
    sview qs, ks, vs;
    if (!resolve_qkv(c, r, 1, B, qs, ks, vs)) return false;
    for (const sview * v : { &qs, &ks, &vs }) if (v->nb[2] % 4 != 0 || v->nb[3] % 4 != 0) return false;
    if (x2->ne[0] != D || x2->ne[1] != H || x2->ne[2] != 1 || x2->ne[3] != B || !ggml_is_contiguous(x2)) return false;
    std::vector<int> members;
    if (!collect_attention_interior(an, pos, c, r, false, members)) return false;
    fill_attention_group(an, c, r, qs, ks, vs, members, grp);
    grp.a.T = 1;   // (the row strides are never used)
    grp.B = (int) B;
    grp.sa.a = grp.a;
    grp.sa.B = (int) B;
    grp.sa.q_bs = qs.nb[3] / 4; grp.sa.k_bs = ks.nb[3] / 4; grp.sa.v_bs = vs.nb[3] / 4;
    grp.sa.kc_bs = (int64_t) kc->nb[3]; grp.sa.vc_bs = (int64_t) vc->nb[3];
    grp.sa.out_bs = H * D;
    grp.sa.mask_bs = mask_per_stream ? C : 0;
    grp.sa.rot_bs = rot_bs;
    grp.sa.index_bs = index_per_stream ? 1 : 0;
    return true;
}

// the decoder-slots form: Tn = 2 rows of B > 1 columns (moshi_hot.cpp transformer_graph_build_columns) - mask [C, Tn, 1, B], index [Tn, 1, B] and the
// RoPE table [D, Tn * B] viewed as [D/2, Tn, 1, B] halves, each column's block dense and one behind the other
static bool match_attention_codec_slots(const analysis & an, int pos, attn_group & grp) {
    attn_chain c; rope_pair r;
    if (!match_attention_chain(an, pos, c) || c.x2->op != GGML_OP_CONT) return false;
    const ggml_tensor * kc = c.kc, * vc = c.vc, * mask = c.mask, * idx = c.idx, * x2 = c.x2;
    const int64_t D = kc->ne[0], C = kc->ne[1], H = kc->ne[2], B = kc->ne[3], Tn = c.qo->ne[1];
    if (B < 2 || Tn < 2 || c.qo->ne[0] != D || c.qo->ne[2] != H || c.qo->ne[3] != B || vc->ne[3] != B) return false;
    if (mask->ne[1] != Tn || mask->ne[2] != 1 || mask->ne[3] != B || ggml_nelements(mask) != C * Tn * B) return false;
    if (idx->ne[0] != Tn || idx->ne[1] != 1 || idx->ne[2] != B || ggml_nelements(idx) != Tn * B) return false;
    if (!match_rope_pair(c, r)) return false;
    if (r.rotr) {
        const ggml_tensor * rotr = r.rotr, * roti = r.roti;
        if (rotr->ne[1] != Tn || rotr->ne[2] != 1 || rotr->ne[3] != B || roti->type != GGML_TYPE_F32 || !ggml_are_same_shape(rotr, roti) || roti->nb[3] != rotr->nb[3] ||
            roti->nb[1] != rotr->nb[1] || (int64_t) rotr->nb[1] != D * 4 || (int64_t) rotr->nb[3] != D * 4 * Tn) return false;
    }
    sview qs, ks, vs;
    if (!resolve_qkv(c, r, Tn, B, qs, ks, vs)) return false;
    for (const sview * v : { &qs, &ks, &vs }) if (v->nb[1] % 4 != 0 || v->nb[2] % 4 != 0 || v->nb[3] % 4 != 0) return false;
    if (x2->ne[0] != D || x2->ne[1] != H || x2->ne[2] != Tn || x2->ne[3] != B || !ggml_is_contiguous(x2)) return false;
    std::vector<int> members;
    if (!collect_attention_interior(an, pos, c, r, false, members)) return false;
    fill_attention_group(an, c, r, qs, ks, vs, members, grp);
    grp.a.T = (int) Tn;
    grp.a.q_ts = qs.nb[1] / 4; grp.a.k_ts = ks.nb[1] / 4; grp.a.v_ts = vs.nb[1] / 4;
    if (grp.mask_node || !k_attn_codec_slots_supported(grp.a)) return false;   // (the mask is a graph input, never a copy made in this graph)
    grp.B = (int) B;
    grp.sa.a = grp.a;
    grp.sa.B = (int) B;
    grp.sa.q_bs = qs.nb[3] / 4; grp.sa.k_bs = ks.nb[3] / 4; grp.sa.v_bs = vs.nb[3] / 4;
    grp.sa.kc_bs = (int64_t) kc->nb[3]; grp.sa.vc_bs = (int64_t) vc->nb[3];
    grp.sa.out_bs = Tn * H * D;
    grp.sa.mask_bs = C * Tn;
    grp.sa.rot_bs = D * Tn;
    grp.sa.index_bs = Tn;
    return true;
}

// B'''. stream slots' mask rows (moshi_hot.cpp transformer_graph_step_slots): for r = 0 .. n-1, in graph order, cont_r = cont(view of a dense row of the
//      bias table, n_el floats at the slot's own column) and cpy(cont_r, view of dst at row r) - n >= 2 rows of one destination, consecutive and in order.
//      Every source is read at the last cpy instead of at its cont: only layout nodes may sit between the members.
struct row_copy_group : group { copy_rows_args a; };
static bool match_row_copies(const analysis & an, int pos, row_copy_group & grp) {
    const ggml_cgraph * g = an.g;
    memset(&grp.a, 0, sizeof(grp.a));
    grp.members.clear();
    const ggml_tensor * dst_root = nullptr, * src_root = nullptr;
    const char * dst0 = nullptr;
    int64_t n_el = 0;
    int rows = 0, i = pos;
    while (i < g->n_nodes && rows < COPY_ROWS_MAX) {
        const ggml_tensor * ct = g->nodes[i];
        if (is_view_op(ct->op) && !an.skip[(size_t) i]) { i++; continue; }   // (the views that feed the next pair)
        if (ct->op != GGML_OP_CONT || an.skip[(size_t) i] || uses_of(an, ct) != 1 || ct->view_src || ct->type != GGML_TYPE_F32 || !ct->data) break;
        const ggml_tensor * sv = ct->src[0];
        if (sv->type != GGML_TYPE_F32 || sv->op != GGML_OP_VIEW || !sv->view_src || !sv->data || sv->nb[0] != 4 || ggml_nelements(sv) != sv->ne[0]) break;
        if (rows == 0) { n_el = sv->ne[0]; src_root = sv->view_src; }
        if (sv->ne[0] != n_el || sv->view_src != src_root || ggml_nelements(ct) != n_el) break;
        // the pair's cpy: the next node that is not a layout op
        int j = i + 1;
        while (j < g->n_nodes && is_view_op(g->nodes[j]->op)) j++;
        if (j >= g->n_nodes || an.skip[(size_t) j]) break;
        const ggml_tensor * cp = g->nodes[j];
        if (cp->op != GGML_OP_CPY || cp->src[0] != ct || cp->type != GGML_TYPE_F32 || !ggml_is_contiguous(cp) || ggml_nelements(cp) != n_el || !cp->data) break;
        const ggml_tensor * root = cp->view_src;
        while (root && root->view_src) root = root->view_src;
        if (!root || root == src_root) break;
        if (rows == 0) { dst_root = root; dst0 = (const char *) cp->data; }
        if (root != dst_root || (const char *) cp->data != dst0 + (size_t) rows * (size_t) n_el * 4) break;
        if ((const char *) cp->data + n_el * 4 > (const char *) root->data + ggml_nbytes(root)) break;
        grp.a.src[rows] = (const float *) sv->data;
        grp.members.push_back(i);
        grp.members.push_back(j);
        grp.emit_pos = j;
        rows++;
        i = j + 1;
    }
    if (rows < 2) return false;
    grp.a.dst = (float *) dst0;
    grp.a.n = n_el;
    grp.a.rows = rows;
    return true;
}

// B'''a. cpy(cont(x), dst): copy the strided source straight into dst (the per-step mask row: cont(view of the bias table) -> cpy into the graph input,
//      transformer.h:1259-1289 - two launches on the LM stream in front of every Temporal graph), matched at the cpy
struct cpy_fold_group : group { tdesc d, x; };
static bool match_cpy_of_cont(const analysis & an, int pos, cpy_fold_group & grp) {
    const ggml_tensor * n = an.g->nodes[pos];
    if (n->op != GGML_OP_CPY) return false;
    const ggml_tensor * ct = n->src[0];
    const int pc = pos_of(an, ct);
    if (ct->op != GGML_OP_CONT || pc < 0 || an.skip[(size_t) pc] || uses_of(an, ct) != 1 || ct->view_src) return false;
    if (ct->type != GGML_TYPE_F32 || n->type != GGML_TYPE_F32 || ct->src[0]->type != GGML_TYPE_F32 || !ggml_are_same_shape(ct, ct->src[0]) ||
        !ggml_are_same_shape(n, ct) || !ggml_is_contiguous(n)) return false;
    // the strided source is read at the cpy's position instead of the cont's: nothing in between may write through an alias (set_rows, a cpy into
    // a view of the same table), or the fold would copy newer data than the cont saw
    for (int j = pc + 1; j < pos; j++) if (writes_through_alias(an.g->nodes[j])) return false;
    grp.members = { pos, pc };
    grp.emit_pos = pos;
    grp.d = make_tdesc(n); grp.x = make_tdesc(ct->src[0]);
    return true;
}

// B'''b. timestep table of add(a, b): one launch (the Temporal graph's RoPE phase: add(arange, offset) -> timestep_embedding), matched at the
//      timestep_embedding. hoist_dst is set when both operands are uploaded leaves (pstep::hoist_dst)
struct timestep_group : group { tdesc d, x; const float * y; int yn, dim, max_period; const char * hoist_dst; size_t hoist_bytes; };
static bool match_timestep_of_add(const analysis & an, int pos, timestep_group & grp) {
    const ggml_tensor * n = an.g->nodes[pos];
    if (n->op != GGML_OP_TIMESTEP_EMBEDDING) return false;
    const ggml_tensor * ad = n->src[0];
    const int pa = pos_of(an, ad);
    if (ad->op != GGML_OP_ADD || pa < 0 || an.skip[(size_t) pa] || uses_of(an, ad) != 1 || ad->view_src || ad->type != GGML_TYPE_F32) return false;
    const ggml_tensor * x = ad->src[0], * y = ad->src[1];
    if (x->type != GGML_TYPE_F32 || y->type != GGML_TYPE_F32 || !ggml_is_contiguous(x) || !ggml_is_contiguous(y) || !ggml_are_same_shape(x, ad) ||
        ggml_nelements(ad) != ad->ne[0] || !(ggml_nelements(y) == ggml_nelements(ad) || ggml_nelements(y) == 1)) return false;
    grp.members = { pos, pa };
    grp.emit_pos = pos;
    grp.d = make_tdesc(n); grp.x = make_tdesc(x);
    grp.y = (const float *) y->data; grp.yn = (int) ggml_nelements(y);
    grp.dim = n->op_params[0]; grp.max_period = n->op_params[1];
    const bool leaves = x->op == GGML_OP_NONE && y->op == GGML_OP_NONE && !x->view_src && !y->view_src;   // (both operands are uploaded leaves)
    grp.hoist_dst = leaves ? (const char *) n->data : nullptr; grp.hoist_bytes = leaves ? ggml_nbytes(n) : 0;
    return true;
}

// B''''. snapshots (moshi_hot.cpp state_graph): a run of cpy(a, b) of one type with nothing but layout nodes between the copies, at least one side of each
//      inside ONE column of a B-column root (B > 1), as one launch. Two forms on one run walk, which differ in what a side must be:
//      ring copies   [D, n, H] row-range views - each head one contiguous run of n x D elements on both sides - a side inside one column of a [D, C, H, B]
//                    ring: one k_ring_copy launch for up to RING_COPY_MAX of them. Bases, head strides and run length are multiples of 16 bytes, and H
//                    and the run length are the same for the whole run.
//      state copies  contiguous unquantised tensors - each side one run of bytes - a side exactly one column of a [len, C, B] root (a carried conv
//                    state): one k_state_copy launch for up to STATE_COPY_MAX of them. Bases and length are multiples of 4 bytes. The run is taken only
//                    if at least two of its jobs are columns of two or more rows (view ne[1] >= 2): a lone column copy (cond_cross in a tts fork) and
//                    1-D row copies (transformer_out, cond_sum) stay the generic copies they always were.
//      A copy that fails its form's test, a side that leaves its root tensor, a source that overlaps its destination, or a copy that touches what an
//      earlier job of the run writes (or writes what one reads) ends the run and stays a generic copy.
struct ring_copy_group : group { ring_copy_args a; };
struct state_copy_group : group { state_copy_args a; };
struct byte_range { const char * lo, * hi; bool overlaps(const byte_range & o) const { return lo < o.hi && o.lo < hi; } };
struct copy_side { byte_range span; bool column; };
// sd.span (the bytes of t) against t's root tensor: false when it leaves the root. sd.column: t is a view inside one column of the root along dimension
// d (ne[d] > 1), in one of two senses:
//   exact = false (ring copies)   the span lies within a column's nb[d] bytes: some rows of every head of one ring column
//   exact = true  (state copies)  the root is contiguous and ends with d, and the span is one whole column of it, first byte to last
static bool copy_side_in_root(const ggml_tensor * t, int d, bool exact, copy_side & sd) {
    const ggml_tensor * root = t;
    while (root->view_src) root = root->view_src;
    const byte_range & sp = sd.span;
    if (!root->data || sp.lo < (const char *) root->data || sp.hi > (const char *) root->data + ggml_nbytes(root)) return false;
    sd.column = false;
    if (root != t && root->ne[d] > 1 && root->nb[d] > 0 && (!exact || (root->ne[3] == 1 && ggml_is_contiguous(root)))) {
        const int64_t col = (int64_t) root->nb[d], off = sp.lo - (const char *) root->data;
        sd.column = exact ? off % col == 0 && sp.hi - sp.lo == col : sp.hi <= (const char *) root->data + (off / col + 1) * col;
    }
    return true;
}
// t as H runs of contiguous bytes inside its root tensor: base span.lo, head stride nb[2], run length *run
static bool ring_copy_side(const ggml_tensor * t, int64_t * run, copy_side & sd) {
    const int64_t es = (int64_t) ggml_type_size(t->type), hs = (int64_t) t->nb[2];
    if (!t->data || ggml_is_quantized(t->type) || t->ne[3] != 1 || (int64_t) t->nb[0] != es || (int64_t) t->nb[1] != t->ne[0] * es) return false;
    *run = t->ne[0] * t->ne[1] * es;
    if (hs < *run) return false;
    sd.span.lo = (const char *) t->data; sd.span.hi = sd.span.lo + (t->ne[2] - 1) * hs + *run;
    return copy_side_in_root(t, 3, false, sd) && ((uintptr_t) sd.span.lo | (uintptr_t) hs | (uintptr_t) *run) % 16 == 0;
}
// t as one run of bytes inside its root tensor
static bool state_copy_side(const ggml_tensor * t, copy_side & sd) {
    if (!t->data || ggml_is_quantized(t->type) || !ggml_is_contiguous(t) || ggml_nbytes(t) == 0) return false;
    sd.span.lo = (const char *) t->data; sd.span.hi = sd.span.lo + ggml_nbytes(t);
    return copy_side_in_root(t, 2, true, sd) && ((uintptr_t) sd.span.lo | (uintptr_t) (sd.span.hi - sd.span.lo)) % 4 == 0;
}
// The run walk from node pos on, for up to max_jobs copies: sides(cp, src, dst) resolves a copy's two sides under its form's conditions, take(cp, src, dst)
// appends the job of a copy the walk has accepted (job grp.members.size()). -> the number of jobs
template <class Sides, class Take> static int walk_copy_run(const analysis & an, int pos, int max_jobs, group & grp, Sides sides, Take take) {
    const ggml_cgraph * g = an.g;
    grp.members.clear();
    std::vector<byte_range> reads, writes;
    for (int i = pos; i < g->n_nodes && (int) grp.members.size() < max_jobs; i++) {
        const ggml_tensor * cp = g->nodes[i];
        if (is_view_op(cp->op) && !an.skip[(size_t) i]) continue;   // (the views that feed the next copy)
        if (cp->op != GGML_OP_CPY || an.skip[(size_t) i] || uses_of(an, cp) != 0) break;
        copy_side sa, sb;
        if (cp->src[0]->type != cp->type || !sides(cp, sa, sb)) break;
        const byte_range & ra = sa.span, & rb = sb.span;
        if (!(sa.column || sb.column) || ra.overlaps(rb)) break;
        bool hazard = false;
        for (const byte_range & w : writes) if (w.overlaps(ra) || w.overlaps(rb)) hazard = true;
        for (const byte_range & r : reads) if (r.overlaps(rb)) hazard = true;
        if (hazard) break;
        take(cp, sa, sb);
        reads.push_back(ra); writes.push_back(rb);
        grp.members.push_back(i);
        grp.emit_pos = i;
    }
    return (int) grp.members.size();
}
static bool match_ring_copies(const analysis & an, int pos, ring_copy_group & grp) {
    ring_copy_args & ar = grp.a;
    memset(&ar, 0, sizeof(ar));
    ar.n_jobs = walk_copy_run(an, pos, RING_COPY_MAX, grp, [&](const ggml_tensor * cp, copy_side & sa, copy_side & sb) {
        const ggml_tensor * a = cp->src[0];
        int64_t run_a = 0, run_b = 0;
        if (a->ne[0] != cp->ne[0] || a->ne[1] != cp->ne[1] || a->ne[2] != cp->ne[2] || cp->ne[2] < 2) return false;
        if (!ring_copy_side(a, &run_a, sa) || !ring_copy_side(cp, &run_b, sb) || run_a != run_b) return false;
        return grp.members.empty() || (cp->ne[2] == ar.H && run_a == ar.run_bytes);
    }, [&](const ggml_tensor * cp, const copy_side & sa, const copy_side & sb) {
        ar.H = (int) cp->ne[2]; ar.run_bytes = cp->ne[0] * cp->ne[1] * (int64_t) ggml_type_size(cp->type);
        ar.job[grp.members.size()] = { sa.span.lo, (char *) sb.span.lo, (int64_t) cp->src[0]->nb[2], (int64_t) cp->nb[2] };
    });
    return ar.n_jobs > 0;
}
static bool match_state_copies(const analysis & an, int pos, state_copy_group & grp) {
    memset(&grp.a, 0, sizeof(grp.a));
    int wide = 0;
    grp.a.n_jobs = walk_copy_run(an, pos, STATE_COPY_MAX, grp, [&](const ggml_tensor * cp, copy_side & sa, copy_side & sb) {
        return state_copy_side(cp->src[0], sa) && state_copy_side(cp, sb) && sa.span.hi - sa.span.lo == sb.span.hi - sb.span.lo;
    }, [&](const ggml_tensor * cp, const copy_side & sa, const copy_side & sb) {
        grp.a.job[grp.members.size()] = { sa.span.lo, (char *) sb.span.lo, (int64_t) (sa.span.hi - sa.span.lo) };
        if ((sa.column && cp->src[0]->ne[1] >= 2) || (sb.column && cp->ne[1] >= 2)) wide++;
    });
    return grp.a.n_jobs > 0 && wide >= 2;
}

// A'. several activation rows against Q4_K weights (batched prompt prefill): the int8-MFMA mat-mul with the activation producer
//     (alpha * rms_norm(x), or silu(h[:n]) * h[n:]) folded into its row quantiser and the residual add into its epilogue.
//     BF16 / F16 weights: the f64-MFMA mat-mul with the same folds in its row converter and epilogue
struct bmm_group : group { std::function<void(hipStream_t)> run; bool float_weights = false, float_acc = false; };
static bool match_batched_mm(const analysis & an, int pos, emitter & em, bmm_group & grp) {
    const ggml_tensor * mm = an.g->nodes[pos];
    if (mm->op != GGML_OP_MUL_MAT) return false;
    const ggml_tensor * w0 = mm->src[0], * x1 = mm->src[1];
    const bool fw = w0->type == GGML_TYPE_BF16 || w0->type == GGML_TYPE_F16;
    if (!(is_qblock(w0->type) || fw) || !ggml_is_contiguous(w0) || w0->ne[2] != 1 || w0->ne[3] != 1) return false;
    if (x1->type != GGML_TYPE_F32 || !ggml_is_contiguous(x1) || mm->type != GGML_TYPE_F32 || !ggml_is_contiguous(mm) || mm->view_src) return false;
    const int64_t K = w0->ne[0], M = w0->ne[1], Tn = ggml_nelements(x1) / K;
    const bool facc = fw && em.c->float_acc != 0;
    if (fw ? !float_batched_ok(w0, Tn, facc) : !k_mm_q4k_batched_supported(w0->type, K, M, Tn)) return false;
    grp.float_weights = fw; grp.float_acc = facc;
    grp.members.assign(1, pos);
    grp.emit_pos = pos;
    int prologue = MV_PLAIN;
    const float * xp = (const float *) x1->data, * alpha = nullptr;
    int64_t x_cs = K;
    float eps = 0.f;
    const ggml_tensor * b = x1;
    while ((b->op == GGML_OP_VIEW || b->op == GGML_OP_RESHAPE) && uses_of(an, b) == 1 && b->src[0]->data == b->data &&
           ggml_nelements(b->src[0]) == ggml_nelements(b) && ggml_is_contiguous(b->src[0])) b = b->src[0];
    if (b->op == GGML_OP_MUL && uses_of(an, b) == 1 && b->view_src == NULL) {
        const ggml_tensor * s0 = b->src[0], * s1 = b->src[1];
        const ggml_tensor * nr = s0->op == GGML_OP_RMS_NORM ? s0 : s1->op == GGML_OP_RMS_NORM ? s1 : nullptr;
        const ggml_tensor * al = nr == s0 ? s1 : s0;
        if (nr && uses_of(an, nr) == 1 && is_f32_vec(al, K) && is_f32_vec(nr->src[0], K * Tn) && nr->src[0]->ne[0] == K) {
            prologue = MV_RMSNORM;
            xp = (const float *) nr->src[0]->data;
            alpha = (const float *) al->data;
            eps = ggml_get_op_params_f32(nr, 0);
            grp.members.push_back(pos_of(an, b)); grp.members.push_back(pos_of(an, nr));
        } else if (s0->op == GGML_OP_UNARY && s0->op_params[0] == GGML_UNARY_OP_SILU && uses_of(an, s0) == 1 && s0->src[0]->op == GGML_OP_VIEW &&
                   s1->op == GGML_OP_VIEW && uses_of(an, s0->src[0]) == 1 && uses_of(an, s1) == 1) {
            const ggml_tensor * l = s0->src[0], * r = s1, * h = l->src[0];
            if (r->src[0] == h && is_f32_vec(h, 2 * K * Tn) && h->ne[0] == 2 * K && l->data == h->data && (const char *) r->data == (const char *) h->data + K * 4 &&
                l->ne[0] == K && r->ne[0] == K && ggml_nelements(l) == K * Tn && ggml_nelements(r) == K * Tn &&
                l->ne[1] == 1 && r->ne[1] == 1 &&
                ((l->nb[2] == h->nb[1] && r->nb[2] == h->nb[1] && l->ne[2] == Tn && r->ne[2] == Tn) ||                                   // prefill: [F, 1, T]
                 (l->ne[2] == 1 && r->ne[2] == 1 && l->nb[3] == h->nb[1] && r->nb[3] == h->nb[1] && l->ne[3] == Tn && r->ne[3] == Tn))) {  // streams: [F, 1, 1, B]
                prologue = MV_GATE_SILU;
                xp = (const float *) h->data;
                x_cs = 2 * K;
                grp.members.push_back(pos_of(an, b)); grp.members.push_back(pos_of(an, s0));
            }
        }
    }
    float * yp = (float *) mm->data;
    const float * res = nullptr;
    {   // residual add, possibly behind the gating's shape fold
        const ggml_tensor * cur = mm, * c = sole_consumer(an, mm);
        while (c && (c->op == GGML_OP_RESHAPE || c->op == GGML_OP_VIEW) && c->data == cur->data && ggml_is_contiguous(c) && ggml_nelements(c) == ggml_nelements(cur)) { cur = c; c = sole_consumer(an, c); }
        if (c && c->op == GGML_OP_ADD && c->type == GGML_TYPE_F32 && ggml_is_contiguous(c) && c->view_src == NULL && ggml_nelements(c) == M * Tn && (c->src[0] == cur || c->src[1] == cur)) {
            const ggml_tensor * other = c->src[0] == cur ? c->src[1] : c->src[0];
            if (other != cur && is_f32_vec(other, M * Tn)) {
                res = (const float *) other->data;
                yp = (float *) c->data;
                grp.members.push_back(pos_of(an, c));
                grp.emit_pos = pos_of(an, c);
            }
        }
    }
    for (int m : grp.members) if (m < 0) return false;
    if (fw && (!aligned16(xp) || (alpha && !aligned16(alpha)))) return false;   // (x_cs is K or 2 K floats, K % 32 == 0: every row is then aligned)
    const char * wp = (const char *) w0->data;
    const int64_t rb = (int64_t) w0->nb[1];
    void * ws = em.ws(fw ? k_mm_f_batched_ws_size(K, Tn) : k_mm_q4k_batched_ws_size(K, Tn));
    const int wt = (int) w0->type;
    if (facc) grp.run = [=](hipStream_t s) { k_mm_f32acc_batched(s, wt, wp, rb, K, M, Tn, xp, x_cs, ws, yp, M, res, M, prologue, alpha, eps); };
    else if (fw) grp.run = [=](hipStream_t s) { k_mm_f_batched(s, wt, wp, rb, K, M, Tn, xp, x_cs, ws, yp, M, res, M, prologue, alpha, eps); };
    else grp.run = [=](hipStream_t s) { k_mm_q4k_batched(s, wt, wp, rb, K, M, Tn, xp, x_cs, ws, yp, M, res, M, prologue, alpha, eps); };
    return true;
}

// B'. cross-attention over a cached condition. THE CHAIN, walked once for both forms from the output node x2 at `pos`, an F32 `out_op` (cont or cpy) of
//     x1 = permute(pv), pv = mul_mat(vt = cont(transpose(vx)), sm), sm = soft_max(kq = mul_mat(kx, qp)) without a mask and with max_bias 0. Guaranteed:
//     x1, pv, vt, its transpose, sm and kq have one consumer each; the five members (x2, pv, vt, sm, kq) are nodes of the graph. What kx / vx / qp / x2 may be
//     is the caller's.
struct xattn_chain { const ggml_tensor * x2, * vx, * sm, * kx, * qp; };
static bool match_cross_attention_chain(const analysis & an, int pos, enum ggml_op out_op, xattn_chain & c, std::vector<int> & members) {
    c.x2 = an.g->nodes[pos];
    if (c.x2->op != out_op || c.x2->type != GGML_TYPE_F32) return false;
    const ggml_tensor * x1 = c.x2->src[0];
    if (x1->op != GGML_OP_PERMUTE || uses_of(an, x1) != 1) return false;
    const ggml_tensor * pv = x1->src[0];
    if (pv->op != GGML_OP_MUL_MAT || uses_of(an, pv) != 1) return false;
    const ggml_tensor * vt = pv->src[0];
    c.sm = pv->src[1];
    if (vt->op != GGML_OP_CONT || uses_of(an, vt) != 1 || vt->src[0]->op != GGML_OP_TRANSPOSE || uses_of(an, vt->src[0]) != 1) return false;
    c.vx = vt->src[0]->src[0];
    if (c.sm->op != GGML_OP_SOFT_MAX || uses_of(an, c.sm) != 1 || c.sm->src[1] != NULL || ggml_get_op_params_f32(c.sm, 1) != 0.0f) return false;
    const ggml_tensor * kq = c.sm->src[0];
    if (kq->op != GGML_OP_MUL_MAT || uses_of(an, kq) != 1) return false;
    c.kx = kq->src[0]; c.qp = kq->src[1];
    members = { pos, pos_of(an, pv), pos_of(an, vt), pos_of(an, c.sm), pos_of(an, kq) };
    for (int m : members) if (m < 0) return false;
    return true;
}

//     B columns of cached state (B-column LM steps; B = 1: the single stream), ending at x2 = cont(..): K / V [D, Tc, H, B], q [D, 1, H, B] over a dense
//     [D * H, B], x2 [D, H, 1, B] - one (head, column) workgroup each
struct xattn_group : group { xattn_args a; };
static bool match_cross_attention(const analysis & an, int pos, xattn_group & grp) {
    xattn_chain c;
    if (!match_cross_attention_chain(an, pos, GGML_OP_CONT, c, grp.members)) return false;
    const ggml_tensor * x2 = c.x2, * kx = c.kx, * vx = c.vx, * qp = c.qp;
    if (kx->type != GGML_TYPE_F32 || vx->type != GGML_TYPE_F32 || !kx->data || !vx->data || pos_of(an, kx) >= 0 || pos_of(an, vx) >= 0) return false;   // cached state, not graph values
    const int64_t D = kx->ne[0], Tc = kx->ne[1], H = kx->ne[2], B = kx->ne[3];
    if (D < 1 || D > 256 || Tc < 1 || H < 1 || B < 1 || B > 65535) return false;
    if (vx->ne[0] != D || vx->ne[1] != Tc || vx->ne[2] != H || vx->ne[3] != B || kx->nb[0] != 4 || vx->nb[0] != 4) return false;
    // q: [D, 1, H(, B)] permuted view of a dense [D * H(, B)] vector
    if (qp->ne[0] != D || qp->ne[1] != 1 || qp->ne[2] != H || qp->ne[3] != B || qp->type != GGML_TYPE_F32 || qp->nb[0] != 4 || (int64_t) qp->nb[2] != D * 4) return false;
    if (B > 1 && (int64_t) qp->nb[3] != D * H * 4) return false;
    const ggml_tensor * qsrc = qp;
    while (is_view_op(qsrc->op) && qsrc->op != GGML_OP_NONE && qsrc->src[0]) { if (uses_of(an, qsrc) != 1) return false; qsrc = qsrc->src[0]; }
    if (!is_f32_vec(qsrc, D * H * B) || qsrc->ne[0] != D * H || qsrc->data != qp->data) return false;
    if (x2->ne[0] != D || x2->ne[1] != H || x2->ne[2] != 1 || x2->ne[3] != B || !ggml_is_contiguous(x2)) return false;
    xattn_args & a = grp.a;
    a.q = (const float *) qp->data;
    a.k = (const char *) kx->data; a.v = (const char *) vx->data;
    a.k_nb1 = (int64_t) kx->nb[1]; a.k_nb2 = (int64_t) kx->nb[2]; a.v_nb1 = (int64_t) vx->nb[1]; a.v_nb2 = (int64_t) vx->nb[2];
    a.H = (int) H; a.D = (int) D; a.Tc = (int) Tc;
    a.scale = ggml_get_op_params_f32(c.sm, 0);
    a.out = (float *) x2->data;
    a.B = (int) B; a.q_cs = D * H; a.out_cs = D * H; a.k_nb3 = (int64_t) kx->nb[3]; a.v_nb3 = (int64_t) vx->nb[3];
    grp.emit_pos = pos;
    return true;
}

//     one job of a replay pass's cross-attention (moshi_hot.cpp cross_attention_jobs), ending at x2 = cpy(.., rows), the copy into the job's rows of the
//     layer's shared [D, H, T] tensor: K_b / V_b = [D, Tc, H] views of one column of the cached [D, Tc, H, B] states, q_j = the job's rows of the layer's
//     query projection [D * H, T] seen as [D, T_j, H]
struct xattn_job_group : group { xattn_args a; xattn_block_job job; int64_t q_rs, out_rs; };
static bool match_cross_attention_job(const analysis & an, int pos, xattn_job_group & grp) {
    xattn_chain c;
    if (!match_cross_attention_chain(an, pos, GGML_OP_CPY, c, grp.members)) return false;
    const ggml_tensor * x2 = c.x2, * kx = c.kx, * vx = c.vx, * qp = c.qp;
    if (!x2->data || !ggml_is_contiguous(x2)) return false;
    // K / V: whole-column views of cached states (leaves of the graph), F32 [D, Tc, H]
    for (const ggml_tensor * t : { kx, vx }) {
        if (t->op != GGML_OP_VIEW || !t->view_src || !t->data || t->type != GGML_TYPE_F32 || uses_of(an, t) != 1) return false;
        const ggml_tensor * root = t->view_src;
        if (pos_of(an, root) >= 0 || !root->data || root->view_src || root->ne[0] != t->ne[0] || root->ne[1] != t->ne[1] || root->ne[2] != t->ne[2]) return false;
        if (t->nb[0] != 4 || t->nb[1] != root->nb[1] || t->nb[2] != root->nb[2] || t->ne[3] != 1) return false;
        const int64_t off = (const char *) t->data - (const char *) root->data;
        if (off < 0 || off % (int64_t) root->nb[3] != 0 || off / (int64_t) root->nb[3] >= root->ne[3]) return false;
    }
    const int64_t D = kx->ne[0], Tc = kx->ne[1], H = kx->ne[2], Tn = qp->ne[1];
    if (D < 1 || D > 256 || Tc < 1 || H < 1 || Tn < 1 || Tn > 64 || vx->ne[0] != D || vx->ne[1] != Tc || vx->ne[2] != H) return false;
    if ((int64_t) kx->nb[1] < D * 4 || (int64_t) kx->nb[2] < Tc * (int64_t) kx->nb[1] || (int64_t) vx->nb[1] < D * 4 || (int64_t) vx->nb[2] < Tc * (int64_t) vx->nb[1]) return false;
    // q: [D, T_j, H] permuted view of T_j rows of a dense [D * H, T] projection
    if (qp->op != GGML_OP_PERMUTE || qp->type != GGML_TYPE_F32 || uses_of(an, qp) != 1 || qp->ne[0] != D || qp->ne[2] != H || qp->ne[3] != 1) return false;
    if (qp->nb[0] != 4 || (int64_t) qp->nb[2] != D * 4 || (int64_t) qp->nb[1] != D * H * 4) return false;
    const ggml_tensor * qv = qp->src[0];
    if (qv->op != GGML_OP_VIEW || uses_of(an, qv) != 1 || qv->data != qp->data) return false;
    const ggml_tensor * qsrc = qv->src[0];
    if (!qsrc->data || qsrc->type != GGML_TYPE_F32 || !ggml_is_contiguous(qsrc) || qsrc->ne[0] != D * H) return false;
    const int64_t q_off = (const char *) qp->data - (const char *) qsrc->data;
    if (q_off < 0 || q_off % (D * H * 4) != 0 || q_off + Tn * D * H * 4 > (int64_t) ggml_nbytes(qsrc)) return false;
    // out: rows of the shared tensor, dense [D, H, T_j], inside its root
    if (x2->ne[0] != D || x2->ne[1] != H || x2->ne[2] != Tn || x2->ne[3] != 1) return false;
    const ggml_tensor * oroot = x2;
    while (oroot->view_src) oroot = oroot->view_src;
    if (!oroot->data || (const char *) x2->data < (const char *) oroot->data || (const char *) x2->data + Tn * D * H * 4 > (const char *) oroot->data + ggml_nbytes(oroot)) return false;
    xattn_args & a = grp.a;
    a.q = nullptr; a.k = nullptr; a.v = nullptr; a.out = nullptr;
    a.k_nb1 = (int64_t) kx->nb[1]; a.k_nb2 = (int64_t) kx->nb[2]; a.v_nb1 = (int64_t) vx->nb[1]; a.v_nb2 = (int64_t) vx->nb[2];
    a.H = (int) H; a.D = (int) D; a.Tc = (int) Tc;
    a.scale = ggml_get_op_params_f32(c.sm, 0);
    grp.job = { (const float *) qp->data, (const char *) kx->data, (const char *) vx->data, (float *) x2->data, (int) Tn };
    grp.q_rs = D * H; grp.out_rs = D * H;
    grp.emit_pos = pos;
    return true;
}

// C. left-deep sum of (scaled) embedding rows ending at node `pos`
struct embed_group : group { embed_sum_args a; };

// B > 1: B columns - rows gathered by B indices [dim, B], times one scale per column [1, B]
static bool match_embed_term(const analysis & an, const ggml_tensor * e, embed_src & out, std::vector<int> & members, int64_t B) {
    const ggml_tensor * gr = e, * scale = nullptr;
    if (e->op == GGML_OP_MUL) {
        gr = e->src[0]; scale = e->src[1];
        if (scale->type != GGML_TYPE_F32 || ggml_nelements(scale) != B || uses_of(an, gr) != 1) return false;
        if (B > 1 && (!ggml_is_contiguous(scale) || scale->ne[0] != 1 || gr->ne[1] != B || !ggml_is_contiguous(gr))) return false;
        members.push_back(pos_of(an, e));
    } else if (B == 1 && e->op == GGML_OP_CONT && e->src[0]->op == GGML_OP_PERMUTE && e->src[0]->src[0]->op == GGML_OP_GET_ROWS) {
        // a single gathered row viewed as [1, K] (moshi_vq_decode, core_vq.h:100-109): same bytes
        const ggml_tensor * pm = e->src[0];
        gr = pm->src[0];
        if (gr->ne[1] != 1 || ggml_nelements(gr) != gr->ne[0] || uses_of(an, pm) != 1 || uses_of(an, gr) != 1) return false;
        members.push_back(pos_of(an, e)); members.push_back(pos_of(an, pm));
    }
    if (gr->op != GGML_OP_GET_ROWS) return false;
    const ggml_tensor * tab = gr->src[0], * idx = gr->src[1];
    if (ggml_nelements(idx) != B || idx->type != GGML_TYPE_I32 || !dense_rows(tab) || (B > 1 && !ggml_is_contiguous(idx))) return false;
    switch (tab->type) { case GGML_TYPE_F32: case GGML_TYPE_F16: case GGML_TYPE_BF16: case GGML_TYPE_Q4_0: case GGML_TYPE_Q8_0: case GGML_TYPE_Q4_K: break; default: return false; }
    const int32_t * ip = (const int32_t *) idx->data;
    if (B == 1 && idx->op == GGML_OP_CONT && uses_of(an, idx) == 1 && idx->src[0]->type == GGML_TYPE_I32 && idx->src[0]->data && pos_of(an, idx) >= 0) {
        ip = (const int32_t *) idx->src[0]->data;   // a one-element copy: read the source
        members.push_back(pos_of(an, idx));
    }
    out = { (const char *) tab->data, (int64_t) tab->nb[1], tab->ne[1], (int) tab->type, ip, scale ? (const float *) scale->data : nullptr };
    members.push_back(pos_of(an, gr));
    return true;
}

static bool match_embed_sum(const analysis & an, int pos, embed_group & grp) {
    const ggml_tensor * top = an.g->nodes[pos];
    if (top->op != GGML_OP_ADD || top->view_src || top->type != GGML_TYPE_F32 || !ggml_is_contiguous(top)) return false;
    if (top->ne[2] != 1 || top->ne[3] != 1) return false;
    // [K] (one row) or [K, B] (B columns: lockstep streams, prompt blocks - every term a row per column, see match_embed_term)
    const int64_t B = top->ne[1] == 1 || top->ne[0] == 1 ? 1 : top->ne[1];
    // walk down the left spine of the chain of adds: adds[d] = adds[d + 1] + terms[d]
    std::vector<const ggml_tensor *> terms, adds;
    const ggml_tensor * cur = top;
    while (cur->op == GGML_OP_ADD && cur->view_src == NULL) {
        const ggml_tensor * l = cur->src[0], * r = cur->src[1];
        if (cur != top && uses_of(an, cur) != 1) break;
        if (uses_of(an, r) != 1 || !ggml_are_same_shape(l, r) || !ggml_are_same_shape(cur, l)) break;
        if (pos_of(an, cur) < 0 || an.skip[(size_t) pos_of(an, cur)]) break;   // (claimed by another group: it is the base then)
        terms.push_back(r);
        adds.push_back(cur);
        cur = l;
    }
    if (terms.size() < 2) return false;
    // embedding rows from the top down; what is left below them - one more embedding row, or any F32 vector of the same shape that something else
    // computes (tts: the demuxed text embedding's two projections, lm_utils.h:48-66) - is the sum's first term
    std::vector<embed_src> srcs(terms.size());
    std::vector<std::vector<int>> mem(terms.size());
    size_t f = 0;
    while (f < terms.size() && match_embed_term(an, terms[f], srcs[f], mem[f], B)) f++;
    if (f < 2) return false;
    const ggml_tensor * base = f == terms.size() ? cur : adds[f];   // adds[f] = the partial sum below the first f rows
    embed_src base_src;
    std::vector<int> base_mem;
    bool base_is_row = false;
    if (f == terms.size() && uses_of(an, cur) == 1 && match_embed_term(an, cur, base_src, base_mem, B)) base_is_row = true;
    if (!base_is_row && B > 1) return false;
    if (!base_is_row) {
        if (base->type != GGML_TYPE_F32 || !ggml_is_contiguous(base) || !ggml_are_same_shape(base, top)) return false;
        // row 0 of a one-row F32 "table": any index is clamped to it (embed_sum_kernel), so the first row's index pointer serves
        base_src = { (const char *) base->data, 0, 1, (int) GGML_TYPE_F32, srcs[0].index, nullptr };
    }
    if (f + 1 < 3 || f + 1 > EMBED_SUM_MAX) return false;
    memset(&grp.a, 0, sizeof(grp.a));
    grp.a.n = (int) f + 1;
    grp.a.K = ggml_nelements(top) / B;
    grp.a.B = (int) B;
    grp.a.out = (float *) top->data;
    grp.a.src[0] = base_src;
    std::vector<int> members = base_mem;
    for (size_t i = 0; i < f; i++) {
        // rows were collected right-to-left (top down); the kernel adds left-to-right
        grp.a.src[1 + i] = srcs[f - 1 - i];
        members.insert(members.end(), mem[f - 1 - i].begin(), mem[f - 1 - i].end());
        members.push_back(pos_of(an, adds[f - 1 - i]));
    }
    grp.members = members;
    grp.emit_pos = pos;
    return true;
}

// C+. the [K, T] input of a persona pass (moshi_hot.cpp persona_pass_input): a left-deep chain of concats along dimension 1 whose pieces are embedding
// sums over their rows (match_embed_sum) and row gathers from dense F32 / BF16 / F16 tensors, matched at the top-most concat -> one k_pass_input launch.
// The token pieces must be ONE sum over the rows of the pass: the same tables in the same order, and every term's index / scale pointers those of one
// array per term with row t of the pass at element t (the pieces take views of it). Anything else is declined and runs as the plain nodes it is.
struct pass_input_group : group { pass_input_args a; };
static bool match_pass_input(const analysis & an, int pos, pass_input_group & grp) {
    const ggml_tensor * top = an.g->nodes[pos];
    auto is_cat = [](const ggml_tensor * t) {
        return t->op == GGML_OP_CONCAT && t->op_params[0] == 1 && t->type == GGML_TYPE_F32 && !t->view_src && ggml_is_contiguous(t) && t->ne[2] == 1 && t->ne[3] == 1;
    };
    if (!is_cat(top) || top->ne[1] > PASS_INPUT_ROWS_MAX) return false;
    std::vector<const ggml_tensor *> pieces;   // right to left
    std::vector<int> members;
    const ggml_tensor * cur = top;
    while (is_cat(cur) && (cur == top || uses_of(an, cur) == 1) && pos_of(an, cur) >= 0 && !an.skip[(size_t) pos_of(an, cur)]) {
        pieces.push_back(cur->src[1]);
        members.push_back(pos_of(an, cur));
        cur = cur->src[0];
    }
    pieces.push_back(cur);
    const int64_t K = top->ne[0], T = top->ne[1];
    pass_input_args & a = grp.a;
    memset(&a, 0, sizeof(a));
    bool have_sum = false;
    int64_t row0 = 0;
    for (size_t pi = pieces.size(); pi-- > 0; ) {   // left to right: rows [row0, row0 + n)
        const ggml_tensor * p = pieces[pi];
        const int64_t n = p->ne[1];
        const int pp = pos_of(an, p);
        if (pp < 0 || an.skip[(size_t) pp] || uses_of(an, p) != 1 || p->type != GGML_TYPE_F32 || !ggml_is_contiguous(p) || p->ne[0] != K || p->ne[2] != 1 || p->ne[3] != 1) return false;
        if (p->op == GGML_OP_GET_ROWS) {
            const ggml_tensor * tab = p->src[0], * idx = p->src[1];
            if (tab->type != GGML_TYPE_F32 && tab->type != GGML_TYPE_BF16 && tab->type != GGML_TYPE_F16) return false;
            if (!dense_rows(tab) || tab->ne[0] != K || !tab->data || idx->type != GGML_TYPE_I32 || !ggml_is_contiguous(idx) || ggml_nelements(idx) != n || !idx->data) return false;
            if (a.n_voices == PASS_INPUT_VOICES_MAX) return false;
            a.voice[a.n_voices] = { (const char *) tab->data, (int64_t) tab->nb[1], tab->ne[1], (const int32_t *) idx->data, (int) tab->type, (int) row0 };
            for (int64_t t = 0; t < n; t++) a.kind[row0 + t] = (int8_t) a.n_voices;
            a.n_voices++;
            members.push_back(pp);
        } else {
            embed_group eg;
            if (!match_embed_sum(an, pp, eg) || eg.a.n > 24 || eg.a.K != K || eg.a.out != (float *) p->data || (int64_t) (eg.a.B > 1 ? eg.a.B : 1) != n) return false;
            // this piece's pointers as those of the whole pass: element row0 of the arrays is the piece's first (only rows of the piece itself are ever read through them).
            // 4 bytes per row on both: the index is a contiguous I32 vector and the scale a contiguous [1, n] F32 tensor (match_embed_term declines anything else at
            // n > 1; a one-row piece reads element 0 of its own operands whatever their strides)
            for (int i = 0; i < eg.a.n; i++) {
                embed_src & e = eg.a.src[i];
                e.index = (const int32_t *) ((uintptr_t) e.index - (uintptr_t) row0 * 4);
                if (e.scale) e.scale = (const float *) ((uintptr_t) e.scale - (uintptr_t) row0 * 4);
            }
            if (!have_sum) { (embed_sum_args &) a = eg.a; have_sum = true; }
            else {
                if (eg.a.n != a.n) return false;
                for (int i = 0; i < eg.a.n; i++) {
                    const embed_src & x = eg.a.src[i], & y = a.src[i];
                    if (x.table != y.table || x.row_bytes != y.row_bytes || x.n_rows != y.n_rows || x.type != y.type || x.index != y.index || x.scale != y.scale) return false;
                }
            }
            for (int64_t t = 0; t < n; t++) a.kind[row0 + t] = -1;
            members.insert(members.end(), eg.members.begin(), eg.members.end());
        }
        row0 += n;
    }
    if (row0 != T) return false;
    a.K = K; a.B = (int) T; a.out = (float *) top->data;
    grp.members = members;
    grp.emit_pos = pos;
    return true;
}

// C'. one embedding row through a small Q8_0 projection (tts: low-rank Depth embeddings): get_rows -> mul_mat [-> cast] as one launch, matched at the mul_mat
struct lowrank_group : group { lowrank_embed_args a; };
static bool match_lowrank_embed(const analysis & an, int pos, lowrank_group & grp) {
    const ggml_tensor * mm = an.g->nodes[pos];
    if (mm->op != GGML_OP_MUL_MAT || mm->type != GGML_TYPE_F32) return false;
    const ggml_tensor * W = mm->src[0], * gr = mm->src[1];
    if (W->type != GGML_TYPE_Q8_0 || !dense_rows(W) || W->ne[2] * W->ne[3] != 1 || gr->op != GGML_OP_GET_ROWS || gr->type != GGML_TYPE_F32) return false;
    const int pg = pos_of(an, gr);
    if (pg < 0 || an.skip[(size_t) pg] || uses_of(an, gr) != 1 || ggml_nelements(gr) != gr->ne[0] || gr->ne[0] != W->ne[0]) return false;
    const ggml_tensor * tab = gr->src[0], * idx = gr->src[1];
    if (ggml_nelements(idx) != 1 || idx->type != GGML_TYPE_I32 || !dense_rows(tab) || !idx->data) return false;
    switch (tab->type) { case GGML_TYPE_F32: case GGML_TYPE_F16: case GGML_TYPE_BF16: case GGML_TYPE_Q4_0: case GGML_TYPE_Q8_0: break; default: return false; }
    const int64_t K = W->ne[0], M = W->ne[1];
    if (K % 32 != 0 || K > 2048 || ggml_nelements(mm) != M || !ggml_is_contiguous(mm)) return false;
    grp.members = { pg, pos };
    grp.emit_pos = pos;
    float * out = (float *) mm->data;
    const ggml_tensor * cp = sole_consumer(an, mm);   // ggml_cast(.., F32) of an F32 tensor: a copy - write its storage directly
    if (cp && cp->op == GGML_OP_CPY && uses_of(an, mm) == 1 && cp->type == GGML_TYPE_F32 && cp->src[0] == mm && ggml_is_contiguous(cp) && cp->view_src == NULL &&
        ggml_are_same_shape(cp, mm) && pos_of(an, cp) >= 0 && !an.skip[(size_t) pos_of(an, cp)]) {
        grp.members.push_back(pos_of(an, cp)); out = (float *) cp->data; grp.emit_pos = pos_of(an, cp);
    }
    grp.a = { (const char *) tab->data, (int64_t) tab->nb[1], tab->ne[1], (int) tab->type, (const int32_t *) idx->data,
              (const char *) W->data, (int64_t) W->nb[1], (int) K, (int) M, out };
    return true;
}

// D. streaming / stateless conv1d (conv.h:50-96, 137-161): [elu] -> concat(prev, x) -> {tail cpy, im2col} -> mul_mat -> reshape
//    [-> + bias] [-> residual + y]  becomes  stream_im2col + conv_tail + one product with the bias/residual epilogue.
struct step_group : group { std::vector<step_fn> steps; sample_args smp; vq_level_args vq; bool has_vq = false; };   // smp / vq: match_sampler's / match_vq_level's arguments

static bool is_elu(const ggml_tensor * t) { return t->op == GGML_OP_UNARY && t->op_params[0] == GGML_UNARY_OP_ELU && t->view_src == NULL; }
// an elu in front of a convolution's input x, all `uses` uses of it the group's: it joins the members and x becomes its input. -> 1 if so, else 0
static int peel_elu(const analysis & an, const ggml_tensor *& x, int uses, std::vector<int> & members) {
    if (!is_elu(x) || uses_of(an, x) != uses || pos_of(an, x) < 0) return 0;
    members.push_back(pos_of(an, x));
    x = x->src[0];
    return 1;
}
// add(x, b) with b a contiguous F32 leaf of OC values behind ne[0] = 1: the bias of a codec convolution (the conv forms also ask for ne[1] = OC, the
// transposed-conv tail never did). -> b, or null
static const ggml_tensor * conv_bias_of(const ggml_tensor * add, const ggml_tensor * x, int64_t OC) {
    if (!add || add->op != GGML_OP_ADD || add->view_src || add->src[0] != x) return nullptr;
    const ggml_tensor * b = add->src[1];
    return b->op == GGML_OP_NONE && b->type == GGML_TYPE_F32 && b->ne[0] == 1 && ggml_nelements(b) == OC && ggml_is_contiguous(b) ? b : nullptr;
}
// cont(transpose(out)) as out's only use, a contiguous F32 [n0, n1]: the group's last launch stores through the cont's strides instead - one launch
// less, the same values. -> the cont (it and the transpose join the members), or null
static const ggml_tensor * transposed_cont_of(const analysis & an, const ggml_tensor * out, int64_t n0, int64_t n1, std::vector<int> & members) {
    const ggml_tensor * trn = uses_of(an, out) == 1 ? sole_consumer(an, out) : nullptr;
    const ggml_tensor * ct = trn && trn->op == GGML_OP_TRANSPOSE && uses_of(an, trn) == 1 ? sole_consumer(an, trn) : nullptr;
    if (!ct || ct->op != GGML_OP_CONT || ct->type != GGML_TYPE_F32 || !ggml_is_contiguous(ct) || !ct->data || ct->ne[0] != n0 || ct->ne[1] != n1 || ggml_nelements(ct) != n0 * n1 ||
        pos_of(an, trn) < 0 || pos_of(an, ct) < 0 || getenv("MI355X_NO_CONV_TRANSPOSE_FOLD")) return nullptr;
    members.push_back(pos_of(an, trn)); members.push_back(pos_of(an, ct));
    return ct;
}
// the head of both conv forms: mm = mul_mat(reshape(im2col(w, .)), reshape(w)), F16 operands, the im2col, its reshape and the product used once each
struct conv_head { const ggml_tensor * ra, * rw, * im, * w; };
static bool match_conv_head(const analysis & an, const ggml_tensor * mm, conv_head & h) {
    if (mm->op != GGML_OP_MUL_MAT) return false;
    h.ra = mm->src[0]; h.rw = mm->src[1];
    if (h.ra->op != GGML_OP_RESHAPE || h.rw->op != GGML_OP_RESHAPE) return false;
    h.im = h.ra->src[0]; h.w = h.rw->src[0];
    if (h.im->op != GGML_OP_IM2COL || h.im->src[0] != h.w || h.im->type != GGML_TYPE_F16 || h.w->type != GGML_TYPE_F16 || !ggml_is_contiguous(h.w)) return false;
    return uses_of(an, h.im) == 1 && uses_of(an, h.ra) == 1 && uses_of(an, mm) == 1;
}

static bool match_conv(const analysis & an, int pos, step_group & grp, emitter & em) {
    const ggml_tensor * mm = an.g->nodes[pos];
    conv_head h;
    if (!match_conv_head(an, mm, h)) return false;
    const ggml_tensor * ra = h.ra, * rw = h.rw, * im = h.im, * w = h.w;
    const int s0 = im->op_params[0], p0 = im->op_params[2], d0 = im->op_params[4];
    if (p0 != 0 || d0 != 1 || im->ne[2] != 1 || im->ne[3] != 1) return false;
    const ggml_tensor * cat = im->src[1];
    const int Kw = (int) w->ne[0], Cin = (int) w->ne[1];
    std::vector<int> members = { pos_of(an, im), pos_of(an, ra), pos_of(an, rw), pos };
    const ggml_tensor * prev = nullptr, * xin = cat;
    int TP = 0;
    if (cat->op == GGML_OP_CONCAT && cat->op_params[0] == 0 && cat->src[0]->op == GGML_OP_NONE) {
        prev = cat->src[0]; xin = cat->src[1];
        TP = (int) prev->ne[0];
        if (prev->type != GGML_TYPE_F32 || !ggml_is_contiguous(prev) || prev->ne[1] != Cin || ggml_nelements(prev) != (int64_t) TP * Cin || !prev->data) return false;
        if (TP > 32 || uses_of(an, cat) != 2) return false;
        // the tail update: cpy(view(cat, last TP), prev)
        const ggml_tensor * tv = nullptr, * tc = nullptr;
        for (int i = pos_of(an, cat) + 1; i < pos; i++) {
            const ggml_tensor * n = an.g->nodes[i];
            if (n->op == GGML_OP_VIEW && n->src[0] == cat) tv = n;
            if (n->op == GGML_OP_CPY && tv && n->src[0] == tv && n->src[1] == prev) tc = n;
        }
        if (!tv || !tc || uses_of(an, tv) != 1 || uses_of(an, tc) != 0) return false;
        if (tv->ne[0] != TP || tv->ne[1] != Cin || (const char *) tv->data - (const char *) cat->data != (int64_t) (cat->ne[0] - TP) * 4) return false;
        members.push_back(pos_of(an, cat)); members.push_back(pos_of(an, tv)); members.push_back(pos_of(an, tc));
    }
    if (xin->type != GGML_TYPE_F32 || xin->ne[1] != Cin || xin->ne[2] != 1 || xin->ne[3] != 1) return false;
    const int pre_elu = peel_elu(an, xin, 1, members);
    if (!xin->data) return false;
    // epilogue
    const ggml_tensor * out = sole_consumer(an, mm);
    if (!out || out->op != GGML_OP_RESHAPE || out->ne[2] != 1) return false;
    members.push_back(pos_of(an, out));
    const int64_t OL = out->ne[0], Cout = out->ne[1];
    mm_epilogue epi;
    memset(&epi, 0, sizeof(epi));
    const ggml_tensor * nx = sole_consumer(an, out);
    if (const ggml_tensor * b = conv_bias_of(nx, out, Cout); b && b->ne[1] == Cout) {
        epi.bias = (const float *) b->data;
        out = nx; members.push_back(pos_of(an, out));
        nx = sole_consumer(an, out);
    }
    if (nx && nx->op == GGML_OP_ADD && !nx->view_src && nx->src[1] == out && nx->src[0] != out && nx->src[0]->type == GGML_TYPE_F32 &&
        ggml_are_same_shape(nx->src[0], out) && nx->src[0]->data) {
        epi.residual = (const char *) nx->src[0]->data; epi.res_nb0 = (int64_t) nx->src[0]->nb[0]; epi.res_nb1 = (int64_t) nx->src[0]->nb[1];
        out = nx; members.push_back(pos_of(an, out));
    }
    if (!ggml_is_contiguous(out) || !out->data || !im->data) return false;
    // cont(transpose(out)) behind a few-position conv (the encoder's last conv feeding the codec transformer): the product, which stores through its
    // destination's strides at that shape, writes the transposed copy in place of its own output - one launch less, the same values
    const ggml_tensor * tcont = OL <= 8 ? transposed_cont_of(an, out, Cout, OL, members) : nullptr;
    for (int m : members) if (m < 0) return false;
    // The panel hand-off below is a side effect on the emitter (this group registers a slot for its output and may claim its producer's): it must only happen
    // for a group build_plan will accept, so the clash check it runs on the returned members is made here first.
    for (int m : members) if (an.skip[(size_t) m]) return false;
    tdesc d_im = make_tdesc(ra), d_w = make_tdesc(rw), d_x = make_tdesc(xin), d_out = make_tdesc(out);
    d_out.ne[0] = OL; d_out.ne[1] = Cout; d_out.ne[2] = d_out.ne[3] = 1;
    if (tcont) { d_out.data = (char *) tcont->data; d_out.nb[0] = (int64_t) tcont->nb[1]; d_out.nb[1] = (int64_t) tcont->nb[0]; }
    float * pv = prev ? (float *) prev->data : nullptr;
    grp.steps.clear();
    if (TP > 0) {   // the tail update rides on the product kernel (it must follow the im2col, which reads the old tail)
        epi.tail_prev = pv; epi.tail_TP = TP; epi.tail_pre_elu = pre_elu; epi.tail_L = (int) xin->ne[0]; epi.tail_C = Cin;
        epi.tail_x = (const char *) xin->data; epi.tail_nb0 = (int64_t) xin->nb[0]; epi.tail_nb1 = (int64_t) xin->nb[1];
    }
    // Without an im2col launch: where x is the output of a conv / transposed-conv group planned before this one, THAT launch writes this conv's F16 operand
    // (the values stream_im2col_kernel would store, at the same places of a plan-owned panel): same products in the same order, bit-identical. Flag 64 or
    // MI355X_CONV_SCATTER=0 keep the im2col launch. (The gathering form - the product reading (tail | act(x)) itself - was built and measured slower than the
    // launch it removes: profiles/r05_ab_implicit_im2col_gather.txt.)
    static const int scatter_on = getenv("MI355X_CONV_SCATTER") ? atoi(getenv("MI355X_CONV_SCATTER")) : 1;
    bool fused = false;
    tdesc d_a = d_im;
    if (scatter_on && !(em.c->flags & 64)) {
        auto it = em.scatter_of.find(xin);
        if (it != em.scatter_of.end() && it->second->panel == nullptr && xin->nb[0] == 4 && (int64_t) xin->nb[1] == xin->ne[0] * 4 && d_im.nb[0] == 2 && d_im.nb[1] == d_im.ne[0] * 2 &&
            OL == d_im.ne[1] && (int64_t) Kw * Cin == d_im.ne[0] && (int64_t) (OL - 1) * s0 + Kw <= TP + xin->ne[0]) {
            conv_scatter * sc = it->second;
            sc->panel = (uint16_t *) em.ws((size_t) d_im.ne[0] * d_im.ne[1] * 2 + 256);
            sc->prev = pv; sc->K = (int) d_im.ne[0]; sc->Kw = Kw; sc->s0 = s0; sc->TP = TP; sc->M = (int) OL; sc->C = Cin; sc->elu = pre_elu;
            d_a.data = (char *) sc->panel;
            fused = true;
        }
    }
    if (!fused && scatter_on && !(em.c->flags & 64) && Kw == 1 && s0 == 1 && TP == 0 && k_mul_mat_is_few_rows(d_im, d_w) && d_im.nb[1] == d_im.ne[0] * 2) {
        // a 1-tap conv over a few positions fed by something else than a conv launch (the RVQ projections): the product converts its rows itself
        epi.af_x = (const char *) xin->data; epi.af_nb0 = (int64_t) xin->nb[0]; epi.af_nb1 = (int64_t) xin->nb[1]; epi.af_elu = pre_elu;
        fused = true;
    }
    if (!fused) grp.steps.push_back([=](hipStream_t s) { k_stream_im2col(s, d_im, pv, TP, d_x, Kw, s0, pre_elu); });
    const conv_scatter * slot = em.scatter_slot(out);
    grp.steps.push_back([=](hipStream_t s) { mm_epilogue e = epi; e.sc = *slot; k_mul_mat(s, d_out, d_a, d_w, nullptr, &e); });
    grp.members = members;
    grp.emit_pos = pos_of(an, tcont ? tcont : out);
    return true;
}

// D'. a codec convolution at B > 1 columns (decoder slots, moshi_hot.cpp conv_1d_bias): im2col [K, OW, B] F16 -> reshape -> mul_mat(., reshape(w)) ->
//     the strided [OW, OC, B] view of the [OW * B, OC] product -> + bias (or cont). The im2col node keeps its own launch (it carries the batch dimension
//     as it is); the product, the view and the add / cont become one launch that stores in the final layout (k_conv_cols).
static bool match_conv_columns(const analysis & an, int pos, step_group & grp) {
    const ggml_tensor * mm = an.g->nodes[pos];
    conv_head h;
    if (!match_conv_head(an, mm, h) || mm->type != GGML_TYPE_F32 || uses_of(an, h.rw) != 1 || !ggml_is_contiguous(h.im)) return false;
    const ggml_tensor * ra = h.ra, * rw = h.rw, * im = h.im, * w = h.w;
    const int64_t K = im->ne[0], OW = im->ne[1], B = im->ne[2], OC = w->ne[2];
    if (B < 2 || im->ne[3] != 1 || w->ne[3] != 1 || w->ne[0] * w->ne[1] != K || !im->data || !w->data) return false;
    if (ra->ne[0] != K || ra->ne[1] != OW * B || rw->ne[0] != K || rw->ne[1] != OC || ra->data != im->data || rw->data != w->data) return false;
    const ggml_tensor * vw = sole_consumer(an, mm);
    if (!vw || vw->op != GGML_OP_VIEW || vw->data != mm->data || vw->ne[0] != OW || vw->ne[1] != OC || vw->ne[2] != B || vw->ne[3] != 1 || vw->nb[0] != 4 ||
        (int64_t) vw->nb[1] != OW * B * 4 || (int64_t) vw->nb[2] != OW * 4 || uses_of(an, vw) != 1) return false;
    const ggml_tensor * out = sole_consumer(an, vw);
    const float * bias = nullptr;
    if (!out) return false;
    if (const ggml_tensor * b = conv_bias_of(out, vw, OC)) { if (b->ne[1] != OC || !b->data) return false; bias = (const float *) b->data; }
    else if (out->op != GGML_OP_CONT) return false;
    if (out->type != GGML_TYPE_F32 || !ggml_is_contiguous(out) || !out->data || out->ne[0] != OW || out->ne[1] != OC || out->ne[2] != B || out->ne[3] != 1) return false;
    if (K > INT32_MAX || OW * B > INT32_MAX || OC > INT32_MAX) return false;
    grp.members = { pos_of(an, ra), pos_of(an, rw), pos, pos_of(an, vw), pos_of(an, out) };
    for (int m : grp.members) if (m < 0 || an.skip[(size_t) m]) return false;
    float * dst = (float *) out->data; const void * ap = im->data, * wp = w->data;
    const int Kn = (int) K, OWn = (int) OW, OCn = (int) OC, Bn = (int) B;
    grp.steps.clear();
    grp.steps.push_back([=](hipStream_t s) { k_conv_cols(s, dst, ap, wp, bias, Kn, OWn, OCn, Bn); });
    grp.emit_pos = pos_of(an, out);
    return true;
}

// E. streaming conv_transpose_1d (conv.h:240-310): [elu] -> conv_transpose_1d -> add_inplace(view lower, view prev tail) -> view full
//    -> cpy(., prev) [-> + bias] -> view(window) -> cont  becomes the partial products + one finishing kernel.
struct convtr_tail { const ggml_tensor * prev, * out; const float * bias; int PT; std::vector<int> members; };

// the streaming tail shared by the dense and the depthwise transposed conv: y is the freshly computed [OLf, OC] block - or, decoder slots, the
// [OLf, OC, B] tensor the B column products were copied into, `lower` then being the one consumer of y that is not a copy's destination
static bool match_convtr_tail(const analysis & an, const ggml_tensor * y, convtr_tail & t, const ggml_tensor * lower_of_columns = nullptr) {
    if (!lower_of_columns && uses_of(an, y) != 1) return false;
    const int64_t OLf = y->ne[0], OC = y->ne[1], B = y->ne[2];
    if (y->ne[3] != 1 || (B != 1 && !lower_of_columns)) return false;
    const ggml_tensor * lower = lower_of_columns ? lower_of_columns : sole_consumer(an, y);
    if (!lower || lower->op != GGML_OP_VIEW || lower->data != y->data || lower->ne[1] != OC || lower->ne[2] != B || lower->nb[1] != y->nb[1] || lower->nb[2] != y->nb[2]) return false;
    const int64_t PT = lower->ne[0];
    const ggml_tensor * ai = sole_consumer(an, lower);
    if (!ai || ai->op != GGML_OP_ADD || ai->src[0] != lower || ai->data != lower->data) return false;
    const ggml_tensor * partial = ai->src[1];
    if (partial->op != GGML_OP_VIEW || partial->src[0]->op != GGML_OP_NONE || uses_of(an, partial) != 1) return false;
    const ggml_tensor * prev = partial->src[0];
    if (prev->type != GGML_TYPE_F32 || !ggml_is_contiguous(prev) || prev->ne[0] != OLf || prev->ne[1] != OC || ggml_nelements(prev) != OLf * OC * B) return false;
    if (partial->ne[0] != PT || partial->ne[1] != OC || partial->ne[2] != B || (const char *) partial->data - (const char *) prev->data != (OLf - PT) * 4 || partial->nb[1] != prev->nb[1] ||
        partial->nb[2] != prev->nb[2]) return false;
    const ggml_tensor * full = sole_consumer(an, ai);
    if (!full || full->op != GGML_OP_VIEW || full->data != y->data || full->ne[0] != OLf || full->ne[1] != OC || full->ne[2] != B) return false;
    const ggml_tensor * cp = sole_consumer(an, full);
    if (!cp || cp->op != GGML_OP_CPY || cp->src[1] != prev) return false;
    const ggml_tensor * cur = sole_consumer(an, cp);
    t.bias = nullptr;
    t.members = { pos_of(an, lower), pos_of(an, partial), pos_of(an, ai), pos_of(an, full), pos_of(an, cp) };
    if (const ggml_tensor * b = conv_bias_of(cur, cp, OC)) {
        t.bias = (const float *) b->data;
        t.members.push_back(pos_of(an, cur));
        cur = sole_consumer(an, cur);
    }
    if (!cur || cur->op != GGML_OP_VIEW || cur->ne[0] != OLf - PT || cur->ne[1] != OC || cur->ne[2] != B || cur->data != cur->src[0]->data) return false;
    const ggml_tensor * out = sole_consumer(an, cur);
    if (!out || out->op != GGML_OP_CONT || !ggml_is_contiguous(out) || !out->data) return false;
    t.members.push_back(pos_of(an, cur)); t.members.push_back(pos_of(an, out));
    t.prev = prev; t.out = out; t.PT = (int) PT;
    return true;
}

static bool match_convtr(const analysis & an, int pos, step_group & grp, emitter & em) {
    const ggml_tensor * ct = an.g->nodes[pos];
    if (ct->op != GGML_OP_CONV_TRANSPOSE_1D) return false;
    const ggml_tensor * w = ct->src[0], * xin = ct->src[1];
    const int K = (int) w->ne[0], OC = (int) w->ne[1], s0 = ct->op_params[0], L = (int) xin->ne[0], PT = K - s0;
    if (PT <= 0 || PT > L * s0 || xin->type != GGML_TYPE_F32 || !(w->type == GGML_TYPE_F16 || w->type == GGML_TYPE_F32)) return false;
    if ((int64_t) w->nb[1] != (int64_t) w->nb[0] * K) return false;
    convtr_tail t;
    if (!match_convtr_tail(an, ct, t) || t.PT != PT) return false;
    std::vector<int> members = t.members;
    members.push_back(pos);
    const int pre_elu = peel_elu(an, xin, 1, members);
    if (!xin->data) return false;
    for (int m : members) if (m < 0) return false;
    for (int m : members) if (an.skip[(size_t) m]) return false;   // (as in match_conv: no slot is registered for a group build_plan would drop)
    void * ws = em.ws(k_conv_transpose_1d_ws_size(w, xin));
    const tdesc d_w = make_tdesc(w), d_x = make_tdesc(xin), d_out = make_tdesc(t.out);
    float * pv = (float *) t.prev->data;
    const float * bias = t.bias;
    grp.steps.clear();
    const conv_scatter * slot = ggml_is_contiguous(t.out) && t.out->type == GGML_TYPE_F32 ? em.scatter_slot(t.out) : nullptr;
    grp.steps.push_back([=](hipStream_t s) {
        const int nsplit = k_conv_transpose_1d_partial(s, d_w, d_x, ws, pre_elu);
        k_convtr_finish(s, d_out, pv, bias, ws, K, OC, L, s0, nsplit, slot);
    });
    grp.members = members;
    grp.emit_pos = pos_of(an, t.out);
    return true;
}

// E'. the same at B columns (decoder slots, moshi_hot.cpp streaming_conv_transpose): for b = 0 .. B - 1, in graph order, conv_transpose_1d(w, view of
//     column b of x) copied into column b of one [OLf, OC, B] tensor y that no node computes, then the streaming tail ONCE over the B columns of y and of
//     prev. Matched at column 0's conv_transpose_1d; all of it becomes one partial launch over the B x L positions and one finish launch (k_convtr_cols).
static bool match_convtr_columns(const analysis & an, int pos, step_group & grp, emitter & em) {
    const ggml_cgraph * g = an.g;
    const ggml_tensor * ct0 = g->nodes[pos];
    if (ct0->op != GGML_OP_CONV_TRANSPOSE_1D || uses_of(an, ct0) != 1) return false;
    const ggml_tensor * cp0 = sole_consumer(an, ct0);
    if (!cp0 || cp0->op != GGML_OP_CPY || cp0->src[0] != ct0 || cp0->src[1]->op != GGML_OP_VIEW) return false;
    const ggml_tensor * y = cp0->src[1]->src[0];
    if (y->op != GGML_OP_NONE || pos_of(an, y) >= 0 || y->type != GGML_TYPE_F32 || !ggml_is_contiguous(y) || !y->data || y->ne[3] != 1 || cp0->src[1]->data != y->data) return false;
    const ggml_tensor * w = ct0->src[0], * xv0 = ct0->src[1];
    if (xv0->op != GGML_OP_VIEW) return false;
    const ggml_tensor * x = xv0->src[0];
    const int64_t B = y->ne[2];
    const int K = (int) w->ne[0], OC = (int) w->ne[1], s0 = ct0->op_params[0], L = (int) xv0->ne[0], PT = K - s0;
    if (B < 2 || x->ne[2] != B || x->ne[3] != 1 || x->ne[0] != L || x->ne[1] != w->ne[2] || xv0->data != x->data || xv0->nb[1] != x->nb[1] || x->type != GGML_TYPE_F32 || !x->data) return false;
    if (PT <= 0 || PT > L * s0 || !(w->type == GGML_TYPE_F16 || w->type == GGML_TYPE_F32) || (int64_t) w->nb[1] != (int64_t) w->nb[0] * K) return false;
    if (y->ne[0] != (int64_t) (L - 1) * s0 + K || y->ne[1] != OC) return false;
    // the B products and copies, consecutive in graph order
    std::vector<int> members;
    int at = pos;
    for (int64_t b = 0; b < B; b++) {
        // (view of x's column, conv_transpose_1d, view of y's column, cpy - the two views in either order)
        int p_ct = -1;
        for (int i = at; i < g->n_nodes && i < at + 4; i++) if (g->nodes[i]->op == GGML_OP_CONV_TRANSPOSE_1D) { p_ct = i; break; } else if (g->nodes[i]->op != GGML_OP_VIEW) break;
        if (p_ct < 0) return false;
        const ggml_tensor * ct = g->nodes[p_ct];
        const ggml_tensor * cp = uses_of(an, ct) == 1 ? sole_consumer(an, ct) : nullptr;
        if (!cp || cp->op != GGML_OP_CPY || cp->src[0] != ct || uses_of(an, cp) != 0 || pos_of(an, cp) > p_ct + 2) return false;
        const ggml_tensor * xv = ct->src[1], * yv = cp->src[1];
        if (ct->src[0] != w || ct->op_params[0] != s0 || xv->op != GGML_OP_VIEW || xv->src[0] != x || uses_of(an, xv) != 1 || xv->ne[0] != L || xv->ne[1] != x->ne[1] || xv->nb[1] != x->nb[1] ||
            (const char *) xv->data - (const char *) x->data != b * (int64_t) x->nb[2]) return false;
        if (yv->op != GGML_OP_VIEW || yv->src[0] != y || uses_of(an, yv) != 1 || yv->ne[0] != y->ne[0] || yv->ne[1] != OC || yv->nb[1] != y->nb[1] ||
            (const char *) yv->data - (const char *) y->data != b * (int64_t) y->nb[2]) return false;
        for (const ggml_tensor * t : { xv, ct, yv, cp }) members.push_back(pos_of(an, t));
        at = pos_of(an, cp) + 1;
    }
    // the tail's first node: the consumer of y behind the copies that is not a copy's destination
    const ggml_tensor * lower = nullptr;
    for (int i = at; i < g->n_nodes && i < at + 4 && !lower; i++) if (g->nodes[i]->op == GGML_OP_VIEW && g->nodes[i]->src[0] == y) lower = g->nodes[i];
    if (!lower || uses_of(an, y) != (int) B + 1) return false;
    convtr_tail t;
    if (!match_convtr_tail(an, y, t, lower) || t.PT != PT) return false;
    for (int m : t.members) members.push_back(m);
    const ggml_tensor * xin = x;
    const int pre_elu = peel_elu(an, xin, (int) B, members);
    if (!xin->data || xin->type != GGML_TYPE_F32 || xin->ne[2] != B) return false;
    if (t.out->type != GGML_TYPE_F32 || t.out->ne[0] != (int64_t) L * s0 || t.out->ne[1] != OC || t.out->ne[2] != B) return false;
    for (int m : members) if (m < 0 || an.skip[(size_t) m]) return false;
    void * ws = em.ws(k_convtr_cols_ws_size(w, L, B));
    const tdesc d_w = make_tdesc(w), d_x = make_tdesc(xin), d_out = make_tdesc(t.out);
    float * pv = (float *) t.prev->data;
    const float * bias = t.bias;
    grp.steps.clear();
    grp.steps.push_back([=](hipStream_t s) { k_convtr_cols(s, d_out, pv, bias, d_w, d_x, s0, pre_elu, ws); });
    grp.members = members;
    grp.emit_pos = pos_of(an, t.out);
    return true;
}

// E2. depthwise streaming conv_transpose_1d on a single frame (the 12.5 -> 25 Hz upsampler, conv.h:262-278): one multiply per
//     kernel tap, concatenated, then the same streaming tail
static bool match_dw_convtr(const analysis & an, int pos, step_group & grp) {
    const ggml_tensor * y = an.g->nodes[pos];
    if (y->op != GGML_OP_CONCAT || y->op_params[0] != 0 || y->type != GGML_TYPE_F32) return false;
    std::vector<const ggml_tensor *> pieces;
    std::vector<int> members;
    const ggml_tensor * cur = y;
    while (cur->op == GGML_OP_CONCAT && cur->op_params[0] == 0) {
        if (cur != y && uses_of(an, cur) != 1) return false;
        pieces.insert(pieces.begin(), cur->src[1]);
        members.push_back(pos_of(an, cur));
        cur = cur->src[0];
    }
    pieces.insert(pieces.begin(), cur);
    const int K = (int) pieces.size();
    if (K < 2 || K > 16 || y->ne[0] != K || y->ne[2] != 1 || y->ne[3] != 1) return false;   // (one column: the B-column upsample of decoder slots runs node by node)
    const int64_t C = y->ne[1];
    const ggml_tensor * x = nullptr, * w = nullptr;
    for (int k = 0; k < K; k++) {
        const ggml_tensor * pc = pieces[(size_t) k];
        if (pc->op != GGML_OP_MUL || pc->view_src || uses_of(an, pc) != 1 || pc->ne[0] != 1 || pc->ne[1] != C) return false;
        const ggml_tensor * sub = pc->src[1];
        if (sub->op != GGML_OP_VIEW || sub->type != GGML_TYPE_F32 || sub->ne[0] != 1 || sub->ne[1] != C) return false;
        if (k == 0) { x = pc->src[0]; w = sub->src[0]; }
        if (pc->src[0] != x || sub->src[0] != w || (const char *) sub->data - (const char *) w->data != (int64_t) k * (int64_t) w->nb[0] || sub->nb[1] != w->nb[2]) return false;
        members.push_back(pos_of(an, pc)); members.push_back(pos_of(an, sub));
    }
    if (!x || x->type != GGML_TYPE_F32 || x->ne[0] != 1 || x->ne[1] != C || !x->data || w->ne[0] != K || w->nb[0] != 4) return false;
    convtr_tail t;
    if (!match_convtr_tail(an, y, t) || t.PT >= K) return false;
    for (int m : t.members) members.push_back(m);
    for (int m : members) if (m < 0) return false;
    const char * xp = (const char *) x->data; const int64_t x_cs = (int64_t) x->nb[1];
    const char * wp = (const char *) w->data; const int64_t w_cs = (int64_t) w->nb[2];
    float * pv = (float *) t.prev->data; const float * bias = t.bias; float * out = (float *) t.out->data;
    const int PT = t.PT, Cn = (int) C;
    // cont(transpose(out)) behind it (the decoder's upsampler feeding the codec transformer): written directly, as above
    int64_t out_cs = K - PT, out_ks = 1;
    const ggml_tensor * emit = t.out;
    if (const ggml_tensor * ct = transposed_cont_of(an, t.out, C, K - PT, members)) { out = (float *) ct->data; out_cs = 1; out_ks = C; emit = ct; }
    grp.steps.clear();
    grp.steps.push_back([=](hipStream_t s) { k_dw_convtr_frame(s, out, pv, bias, xp, x_cs, wp, w_cs, K, PT, Cn, out_cs, out_ks); });
    grp.members = members;
    grp.emit_pos = pos_of(an, emit);
    return true;
}

// F. one level of the residual-VQ encoder (core_vq.h:27-56 + 171-194): the whole distance / argmax / gather / residual chain
static const ggml_tensor * find_consumer(const analysis & an, const ggml_tensor * t, enum ggml_op op, int nth = 0) {
    for (int i = pos_of(an, t) + 1; i < an.g->n_nodes; i++) {
        const ggml_tensor * n = an.g->nodes[i];
        if (n->op != op) continue;
        bool uses = false;
        for (int s = 0; s < GGML_MAX_SRC; s++) if (n->src[s] == t && n != t) uses = true;
        if (uses && nth-- == 0) return n;
    }
    return nullptr;
}

// The chain both forms of a level share, walked up from the argmax at pos:
//     argmax(div(num, add(reshape(sum_rows(mul(d, d))), addc))), d = sub(repeat(emb), reshape(repeat(reshape(cont(L(resid)))))), L the form's layout node
// with the checks on the codebook, num (one value per code and column) and addc, and the F32 cast that consumes the codes. A level is emitted at that
// cast: everything the kernel reads precedes the argmax, and the next residual is only consumed after its own (later) position; tensors never share
// storage (ggml_backend_alloc_ctx_tensors). members: the chain and the cast.
struct vq_chain {
    const ggml_tensor * am, * dv, * rs, * sr, * rb, * ra2, * ra, * ra0, * ac, * xp, * emb, * num, * addc, * resid, * cs;
    int64_t D, NC;
    std::vector<int> members;
    bool one_use(const analysis & an, const ggml_tensor * t, enum ggml_op op) const { return t && t->op == op && !t->view_src && uses_of(an, t) == 1; }
    bool layout_use(const analysis & an, const ggml_tensor * t, enum ggml_op op) const { return t && t->op == op && uses_of(an, t) == 1; }
    // kernel arguments of either form: the codebook, the two constants, the codes as F32 and I32, the next residual (null at the last level)
    template <class A> void fill(A & a, float * resid_out) const {
        a.emb = (const char *) emb->data; a.emb_row_bytes = (int64_t) emb->nb[1]; a.D = (int) D; a.NC = (int) NC;
        a.add_c = (const float *) addc->data; a.num = (const float *) num->data;
        a.resid_out = resid_out; a.idx_f = (float *) cs->data; a.idx_i = (int32_t *) am->data;
    }
};
static bool walk_vq_chain(const analysis & an, int pos, enum ggml_op layout, vq_chain & c) {
    c.am = an.g->nodes[pos];
    if (c.am->op != GGML_OP_ARGMAX) return false;
    c.dv = c.am->src[0];
    if (!c.one_use(an, c.dv, GGML_OP_DIV)) return false;
    c.num = c.dv->src[0];
    const ggml_tensor * ad = c.dv->src[1];
    if (!c.one_use(an, ad, GGML_OP_ADD)) return false;
    c.rs = ad->src[0]; c.addc = ad->src[1];
    if (!c.layout_use(an, c.rs, GGML_OP_RESHAPE)) return false;
    c.sr = c.rs->src[0];
    if (!c.one_use(an, c.sr, GGML_OP_SUM_ROWS)) return false;
    const ggml_tensor * sq = c.sr->src[0];
    if (!c.one_use(an, sq, GGML_OP_MUL) || sq->src[0] != sq->src[1]) return false;
    const ggml_tensor * df = sq->src[0];
    if (!c.one_use(an, df, GGML_OP_SUB)) return false;
    c.rb = df->src[0]; c.ra2 = df->src[1];
    if (!c.one_use(an, c.rb, GGML_OP_REPEAT) || !c.layout_use(an, c.ra2, GGML_OP_RESHAPE)) return false;
    c.emb = c.rb->src[0]; c.ra = c.ra2->src[0];
    if (!c.one_use(an, c.ra, GGML_OP_REPEAT)) return false;
    c.ra0 = c.ra->src[0];
    if (!c.layout_use(an, c.ra0, GGML_OP_RESHAPE)) return false;
    c.ac = c.ra0->src[0];
    if (!c.one_use(an, c.ac, GGML_OP_CONT)) return false;
    c.xp = c.ac->src[0];
    if (!c.layout_use(an, c.xp, layout)) return false;
    c.resid = c.xp->src[0];
    c.D = c.emb->ne[0]; c.NC = c.emb->ne[1];
    if (c.emb->op != GGML_OP_NONE || c.emb->type != GGML_TYPE_F32 || !dense_rows(c.emb) || c.D != 256 || c.NC > 4096) return false;
    if (c.num->op != GGML_OP_NONE || c.num->type != GGML_TYPE_F32 || ggml_nelements(c.num) != c.NC * ggml_nelements(c.am) || !ggml_is_contiguous(c.num)) return false;
    if (c.addc->op != GGML_OP_NONE || c.addc->type != GGML_TYPE_F32 || ggml_nelements(c.addc) != 1) return false;
    // consumers of the codes: the F32 cast (always) and, in each form's own shape, the centroid gather feeding the next residual (all but the last level)
    c.cs = find_consumer(an, c.am, GGML_OP_CPY);
    if (!c.cs || c.cs->type != GGML_TYPE_F32 || c.cs->src[0] != c.am || c.cs->view_src) return false;
    c.members = { pos };
    for (const ggml_tensor * t : { c.dv, ad, c.rs, c.sr, sq, df, c.rb, c.ra2, c.ra, c.ra0, c.ac, c.xp, c.cs }) c.members.push_back(pos_of(an, t));
    for (int m : c.members) if (m < 0) return false;
    return c.members.back() >= pos;
}
// the next residual behind the gathered centroids qc: sub(resid, qc), the residual's only other use; tail joins the members
static float * vq_next_residual(const analysis & an, vq_chain & c, const ggml_tensor * qc, std::initializer_list<const ggml_tensor *> tail) {
    const ggml_tensor * sb = sole_consumer(an, qc);
    if (!sb || sb->op != GGML_OP_SUB || sb->view_src || sb->src[0] != c.resid || sb->src[1] != qc || !ggml_is_contiguous(sb) || !sb->data) return nullptr;
    if (uses_of(an, c.resid) != 2 || pos_of(an, sb) < 0) return nullptr;
    for (const ggml_tensor * t : tail) { if (pos_of(an, t) < 0) return nullptr; c.members.push_back(pos_of(an, t)); }
    c.members.push_back(pos_of(an, sb));
    return (float *) sb->data;
}

static bool match_vq_level(const analysis & an, int pos, step_group & grp, emitter & em) {
    vq_chain c;
    if (ggml_nelements(an.g->nodes[pos]) != 1 || !walk_vq_chain(an, pos, GGML_OP_PERMUTE, c)) return false;
    const ggml_tensor * am = c.am, * resid = c.resid;
    const int64_t D = c.D, NC = c.NC;
    if (resid->type != GGML_TYPE_F32 || resid->ne[0] != 1 || resid->ne[1] != D || ggml_nelements(resid) != D || !resid->data) return false;
    if (ggml_nelements(c.rb) != D * NC || ggml_nelements(c.ra) != D * NC || ggml_nelements(c.dv) != NC) return false;
    float * resid_out = nullptr;
    const ggml_tensor * ci = find_consumer(an, am, GGML_OP_CONT);   // cont -> get_rows -> permute -> cont -> sub
    if (ci) {
        if (uses_of(an, am) != 2 || uses_of(an, ci) != 1) return false;
        const ggml_tensor * gr = sole_consumer(an, ci);
        if (!c.one_use(an, gr, GGML_OP_GET_ROWS) || gr->src[0] != c.emb || gr->src[1] != ci) return false;
        const ggml_tensor * pm = sole_consumer(an, gr);
        if (!c.layout_use(an, pm, GGML_OP_PERMUTE)) return false;
        const ggml_tensor * qc = sole_consumer(an, pm);
        if (!c.one_use(an, qc, GGML_OP_CONT)) return false;
        resid_out = vq_next_residual(an, c, qc, { ci, gr, pm, qc });
        if (!resid_out) return false;
    } else if (uses_of(an, am) != 1) return false;
    char * ws = (char *) em.ws(VQ_LEVEL_WS_BYTES);
    HIP_CHECK(hipMemsetAsync(ws, 0, VQ_LEVEL_WS_BYTES, em.c->stream));   // stream-ordered behind the block's previous user (plans are built outside capture)
    vq_level_args a;
    c.fill(a, resid_out);
    a.resid = (const char *) resid->data; a.resid_stride = (int64_t) resid->nb[1];
    a.cand_val = (float *) ws; a.cand_idx = (int32_t *) (ws + 1024); a.counter = (unsigned *) (ws + 2048);
    grp.steps.clear();
    grp.steps.push_back([=](hipStream_t s) { k_vq_level(s, a); });
    grp.members = c.members;
    grp.emit_pos = pos_of(an, c.cs);
    grp.vq = a; grp.has_vq = true;
    return true;
}

// F'. the same level at B > 1 columns (encoder slots, moshi_hot.cpp rvq_encode_columns): the B residuals [1, D, B] go through codebook_encode as its
//     ane1 = B rows - distances [NC, B], argmax [B] - and vq_decode gathers the B centroids as [1, D, B]; one k_vq_level_cols launch for all columns.
//     has_vq stays unset: the multi-level chain (vq_chain_kernel) takes single-column levels only.
static bool match_vq_level_columns(const analysis & an, int pos, step_group & grp, emitter & em) {
    const ggml_tensor * am = an.g->nodes[pos];
    const int64_t B = am->ne[0];
    vq_chain c;
    if (B < 2 || B > VQ_COLS_MAX_B || ggml_nelements(am) != B || !am->data || !walk_vq_chain(an, pos, GGML_OP_RESHAPE, c)) return false;
    auto shape = [](const ggml_tensor * t, int64_t n0, int64_t n1, int64_t n2) { return t->ne[0] == n0 && t->ne[1] == n1 && t->ne[2] == n2 && t->ne[3] == 1; };
    const ggml_tensor * emb = c.emb, * resid = c.resid, * cs = c.cs;
    const int64_t D = c.D, NC = c.NC;
    if (NC < 1 || emb->ne[2] != 1 || emb->ne[3] != 1 || !emb->data || !c.num->data || !c.addc->data) return false;
    if (resid->type != GGML_TYPE_F32 || !shape(resid, 1, D, B) || !ggml_is_contiguous(resid) || !resid->data || ((uintptr_t) resid->data & 15)) return false;
    // row b * NC + c of the difference is centroid c against residual b
    if (!shape(c.xp, D, B, 1) || !shape(c.ac, D, B, 1) || !shape(c.ra0, D, 1, B) || !shape(c.ra, D, NC, B) || !shape(c.ra2, D, NC * B, 1) || !shape(c.rb, D, NC * B, 1) ||
        !shape(c.sr, 1, NC * B, 1) || !shape(c.rs, NC, B, 1) || !shape(c.dv, NC, B, 1)) return false;
    if (!ggml_is_contiguous(cs) || ggml_nelements(cs) != B || !cs->data) return false;
    float * resid_out = nullptr;
    const ggml_tensor * i2 = find_consumer(an, am, GGML_OP_RESHAPE);   // reshape -> cont -> reshape -> get_rows -> reshape -> permute -> cont -> sub
    if (i2) {
        if (uses_of(an, am) != 2 || uses_of(an, i2) != 1) return false;
        const ggml_tensor * ci = sole_consumer(an, i2);
        if (!c.one_use(an, ci, GGML_OP_CONT)) return false;
        const ggml_tensor * r1 = sole_consumer(an, ci);
        if (!c.layout_use(an, r1, GGML_OP_RESHAPE) || r1->ne[0] != B || ggml_nelements(r1) != B) return false;
        const ggml_tensor * gr = sole_consumer(an, r1);
        if (!c.one_use(an, gr, GGML_OP_GET_ROWS) || gr->src[0] != emb || gr->src[1] != r1) return false;
        const ggml_tensor * r3 = sole_consumer(an, gr);
        if (!c.layout_use(an, r3, GGML_OP_RESHAPE)) return false;
        const ggml_tensor * pm = sole_consumer(an, r3);
        if (!c.layout_use(an, pm, GGML_OP_PERMUTE)) return false;
        const ggml_tensor * qc = sole_consumer(an, pm);
        if (!c.one_use(an, qc, GGML_OP_CONT) || !shape(qc, 1, D, B)) return false;
        resid_out = vq_next_residual(an, c, qc, { i2, ci, r1, gr, r3, pm, qc });
        if (!resid_out || !shape(sole_consumer(an, qc), 1, D, B) || ((uintptr_t) resid_out & 15)) return false;
    } else if (uses_of(an, am) != 1) return false;
    const size_t ws_bytes = k_vq_level_cols_ws_size((int) NC, (int) B);
    char * ws = (char *) em.ws(ws_bytes);
    HIP_CHECK(hipMemsetAsync(ws, 0, ws_bytes, em.c->stream));   // stream-ordered behind the block's previous user (plans are built outside capture)
    const size_t n_cand = (ws_bytes - 256) / 8;
    vq_level_cols_args a;
    c.fill(a, resid_out);
    a.B = (int) B;
    a.resid = (const char *) resid->data; a.resid_col_bytes = (int64_t) resid->nb[2];
    a.counter = (unsigned *) ws; a.cand_val = (float *) (ws + 256); a.cand_idx = (int32_t *) (ws + 256 + n_cand * 4);
    grp.steps.clear();
    grp.steps.push_back([=](hipStream_t s) { k_vq_level_cols(s, a); });
    grp.members = c.members;
    grp.emit_pos = pos_of(an, cs);
    return true;
}

// G. a tree of concats / layout nodes over one-element F32 tensors, optionally cast to I32 at the top (the RVQ encoder's code
//    vector: vq.h:32-45, 97-114): one gather instead of a copy per concat
static bool vector_like(const ggml_tensor * t) {
    int big = 0;
    for (int i = 0; i < 4; i++) if (t->ne[i] > 1) big++;
    return big <= 1;
}
static bool collect_scalar_leaves(const analysis & an, const ggml_tensor * t, bool top, std::vector<const ggml_tensor *> & leaves, std::vector<int> & members) {
    if (!vector_like(t) || t->type != GGML_TYPE_F32) return false;
    if (ggml_nelements(t) == 1 && t->op != GGML_OP_CONCAT) {
        const ggml_tensor * base = t;
        while ((base->op == GGML_OP_PERMUTE || base->op == GGML_OP_RESHAPE || base->op == GGML_OP_VIEW) && pos_of(an, base) >= 0) {
            if (uses_of(an, base) != 1) break;
            members.push_back(pos_of(an, base));
            base = base->src[0];
            if (ggml_nelements(base) != 1) return false;
        }
        if (!t->data) return false;
        leaves.push_back(t);
        return true;
    }
    if (!top && uses_of(an, t) != 1) return false;
    if (pos_of(an, t) < 0) return false;
    if (t->op == GGML_OP_CONCAT) {
        if (t->view_src) return false;
        members.push_back(pos_of(an, t));
        return collect_scalar_leaves(an, t->src[0], false, leaves, members) && collect_scalar_leaves(an, t->src[1], false, leaves, members);
    }
    if (t->op == GGML_OP_PERMUTE || t->op == GGML_OP_RESHAPE) {
        members.push_back(pos_of(an, t));
        return collect_scalar_leaves(an, t->src[0], false, leaves, members);
    }
    return false;
}
// G'. the same tree at B > 1 columns (encoder slots): concats along dim 1 of [1, k, B] tensors whose leaves are reshapes [1, 1, B] of B-element F32
//     tensors (a level's codes), optionally cast to I32 at the top - dst[b * n + i] = leaf i's element b, one launch.
static bool collect_column_leaves(const analysis & an, const ggml_tensor * t, bool top, int64_t B, std::vector<const ggml_tensor *> & leaves, std::vector<int> & members) {
    if (t->type != GGML_TYPE_F32 || t->ne[0] != 1 || t->ne[2] != B || t->ne[3] != 1) return false;
    if (!top && uses_of(an, t) != 1) return false;
    if (pos_of(an, t) < 0) return false;
    if (t->op == GGML_OP_CONCAT) {
        if (t->view_src || t->op_params[0] != 1) return false;
        members.push_back(pos_of(an, t));
        return collect_column_leaves(an, t->src[0], false, B, leaves, members) && collect_column_leaves(an, t->src[1], false, B, leaves, members);
    }
    if (t->op != GGML_OP_RESHAPE || t->ne[1] != 1) return false;
    const ggml_tensor * base = t->src[0];
    if (base->type != GGML_TYPE_F32 || ggml_nelements(base) != B || !ggml_is_contiguous(base) || !base->data || base->data != t->data) return false;
    members.push_back(pos_of(an, t));
    leaves.push_back(base);
    return true;
}
// either tree, matched at its top: one k_gather_scalars launch. -> the number of columns (0 for the single-column tree), -1 for no match. The two forms part
// on the top's shape alone - [1, n, B] with n and B >= 2 is not vector-like - and differ in their leaf collectors; columns_ok = false declines the B-column one
static int match_code_gather(const analysis & an, int pos, bool columns_ok, step_group & grp) {
    const ggml_tensor * top = an.g->nodes[pos];
    const ggml_tensor * tree = top;
    std::vector<int> members;
    if (top->op == GGML_OP_CPY && top->view_src == NULL && top->type == GGML_TYPE_I32 && top->src[0]->type == GGML_TYPE_F32) {
        members.push_back(pos);
        tree = top->src[0];
        if (uses_of(an, tree) != 1) return -1;
    } else if (top->op != GGML_OP_CONCAT) return -1;
    if (!ggml_is_contiguous(top) || !top->data) return -1;
    const bool cols = !vector_like(top);
    const int64_t n = cols ? top->ne[1] : ggml_nelements(top), B = cols ? top->ne[2] : 1;
    std::vector<const ggml_tensor *> leaves;
    if (cols) {
        if (!columns_ok || top->ne[0] != 1 || top->ne[3] != 1 || B < 2 || n < 2 || !ggml_are_same_shape(top, tree)) return -1;
        if (!collect_column_leaves(an, tree, tree == top, B, leaves, members)) return -1;
    } else if (n < 3 || !collect_scalar_leaves(an, tree, tree == top, leaves, members)) return -1;
    if ((int64_t) leaves.size() != n || n > GATHER_MAX) return -1;
    for (int m : members) if (m < 0) return -1;
    gather_args a;
    memset(&a, 0, sizeof(a));
    a.n = (int) n; a.B = (int) B;
    for (int i = 0; i < a.n; i++) a.src[i] = (const float *) leaves[(size_t) i]->data;
    a.dst = top->data;
    a.dst_type = top->type;
    grp.steps.clear();
    grp.steps.push_back([=](hipStream_t s) { k_gather_scalars(s, a); });
    grp.members = members;
    grp.emit_pos = pos;
    return cols ? (int) B : 0;
}

// H. the top-k sampler (moshi_sample_token with temp > 0, sampling.h:4-64), matched at its last node:
//    out = get_rows(cont(permute(idx)), reshape(argmax(div(reshape(permute(get_rows(cont(permute(p)), idx))), noise))))
//    with idx = view(argsort_desc(p), k), p = soft_max(scale(logits, 1 / temp))
static bool match_sampler(const analysis & an, int pos, step_group & grp) {
    const ggml_tensor * out = an.g->nodes[pos];
    if (out->op != GGML_OP_GET_ROWS || out->type != GGML_TYPE_I32 || ggml_nelements(out) != 1) return false;
    auto is = [&](const ggml_tensor * t, enum ggml_op op, int uses) { return t && t->op == op && pos_of(an, t) >= 0 && uses_of(an, t) == uses; };
    const ggml_tensor * cont2 = out->src[0], * nx = out->src[1];
    if (!is(cont2, GGML_OP_CONT, 1) || !is(cont2->src[0], GGML_OP_PERMUTE, 1)) return false;
    const ggml_tensor * irows = cont2->src[0], * idx = irows->src[0];
    if (!is(idx, GGML_OP_VIEW, 2) || !is(idx->src[0], GGML_OP_ARGSORT, 1) || idx->type != GGML_TYPE_I32 || idx->data != idx->src[0]->data) return false;
    const ggml_tensor * srt = idx->src[0], * pr = srt->src[0];
    if (srt->op_params[0] != GGML_SORT_ORDER_DESC || !is(pr, GGML_OP_SOFT_MAX, 2) || pr->src[1] != NULL) return false;
    if (ggml_get_op_params_f32(pr, 0) != 1.0f || ggml_get_op_params_f32(pr, 1) != 0.0f) return false;
    const ggml_tensor * sc = pr->src[0];
    if (!is(sc, GGML_OP_SCALE, 1) || ggml_get_op_params_f32(sc, 1) != 0.0f) return false;
    const ggml_tensor * logits = sc->src[0];
    const int64_t n = pr->ne[0], k = idx->ne[0];
    if (logits->type != GGML_TYPE_F32 || !ggml_is_contiguous(logits) || ggml_nelements(logits) != n || ggml_nelements(pr) != n || !logits->data) return false;
    if (n > SAMPLE_MAX_N || k > SAMPLE_MAX_K || k < 1 || ggml_nelements(idx) != k) return false;
    // the argmax side
    while (nx && (nx->op == GGML_OP_RESHAPE || nx->op == GGML_OP_VIEW) && pos_of(an, nx) >= 0 && uses_of(an, nx) == 1) nx = nx->src[0];
    std::vector<int> members = { pos, pos_of(an, cont2), pos_of(an, irows), pos_of(an, idx), pos_of(an, srt), pos_of(an, pr), pos_of(an, sc) };
    for (const ggml_tensor * t = out->src[1]; t != nx; t = t->src[0]) members.push_back(pos_of(an, t));
    const ggml_tensor * am = nx;
    if (!is(am, GGML_OP_ARGMAX, 1)) return false;
    const ggml_tensor * q = am->src[0];
    if (!is(q, GGML_OP_DIV, 1) || q->view_src) return false;
    const ggml_tensor * noise = q->src[1], * in2 = q->src[0];
    if (noise->type != GGML_TYPE_F32 || ggml_nelements(noise) != k || !ggml_is_contiguous(noise) || !noise->data || pos_of(an, noise) >= 0) return false;
    members.push_back(pos_of(an, am)); members.push_back(pos_of(an, q));
    const ggml_tensor * t = in2;
    while (t && (t->op == GGML_OP_RESHAPE || t->op == GGML_OP_PERMUTE || t->op == GGML_OP_VIEW) && pos_of(an, t) >= 0 && uses_of(an, t) == 1) { members.push_back(pos_of(an, t)); t = t->src[0]; }
    if (!is(t, GGML_OP_GET_ROWS, 1) || t->src[1] != idx) return false;
    members.push_back(pos_of(an, t));
    const ggml_tensor * c1 = t->src[0];
    if (!is(c1, GGML_OP_CONT, 1) || !is(c1->src[0], GGML_OP_PERMUTE, 1) || c1->src[0]->src[0] != pr) return false;
    members.push_back(pos_of(an, c1)); members.push_back(pos_of(an, c1->src[0]));
    for (int m : members) if (m < 0) return false;
    sample_args a;
    a.logits = (const float *) logits->data; a.n = (int) n; a.scale = ggml_get_op_params_f32(sc, 0); a.k = (int) k;
    a.noise = (const float *) noise->data; a.out = (int32_t *) out->data; a.out2 = nullptr;
    // a copy of the token into an I32 slot (the chained Depth graph's token vector, lm.h:527): written by the same launch
    for (int j = pos + 1; j < an.g->n_nodes; j++) {
        const ggml_tensor * cp = an.g->nodes[j];
        if (cp->op == GGML_OP_CPY && cp->src[0] == out && cp->type == GGML_TYPE_I32 && ggml_nelements(cp) == 1 && cp->data && !an.skip[(size_t) j]) {
            a.out2 = (int32_t *) cp->data; members.push_back(j); break;
        }
    }
    grp.steps.clear();
    grp.steps.push_back([=](hipStream_t s) { k_sample_topk(s, a); });
    grp.members = members;
    grp.emit_pos = pos;
    grp.smp = a;
    return true;
}

// H2. the same sampler over the B columns of a B-column LM step (sample_tokens_streams of the frame driver), matched at its last computing node:
//    out [1, 1, B] = get_rows(cont(permute(reshape(idx))), reshape(argmax(div(reshape(get_rows(cont(permute(reshape(p))), idx)), noise [k, B]))))
//    with idx = cont(view(argsort_desc(p), k)) [k, B], p = soft_max(sc) [n, B], sc = scale(logits, 1 / temp) or mul(logits, inv_temp [1, B])
// inv_temp must be a contiguous F32 graph INPUT (no node of the graph is it, views it or copies into it). A trailing cpy of the B tokens into an I32
// vector (the chained Depth graph's token rows) becomes out2. One workgroup per column and none waits for another: no residency planning.
struct sampler_streams_group : group { sample_streams_args a; };
static bool match_sampler_streams(const analysis & an, int pos, sampler_streams_group & grp) {
    sample_streams_args & a = grp.a; std::vector<int> & members = grp.members;
    grp.emit_pos = pos;
    const ggml_tensor * out = an.g->nodes[pos];
    if (out->op != GGML_OP_GET_ROWS || out->type != GGML_TYPE_I32 || out->ne[0] != 1 || out->ne[1] != 1 || out->ne[3] != 1 || !out->data) return false;
    const int64_t B = out->ne[2];
    if (B < 2 || B > SAMPLE_MAX_B) return false;
    auto is = [&](const ggml_tensor * t, enum ggml_op op, int uses) { return t && t->op == op && pos_of(an, t) >= 0 && uses_of(an, t) == uses; };
    members = { pos };
    // a chain of single-use reshapes / views / permutes below t, collected as members; returns the first other node
    auto through = [&](const ggml_tensor * t, bool permute) {
        while (t && (t->op == GGML_OP_RESHAPE || t->op == GGML_OP_VIEW || (permute && t->op == GGML_OP_PERMUTE)) && pos_of(an, t) >= 0 && uses_of(an, t) == 1) {
            members.push_back(pos_of(an, t)); t = t->src[0];
        }
        return t;
    };
    // the index side: cont(permute(reshape(idx)))
    const ggml_tensor * cont2 = out->src[0];
    if (!is(cont2, GGML_OP_CONT, 1)) return false;
    members.push_back(pos_of(an, cont2));
    const ggml_tensor * idx = through(cont2->src[0], true);
    if (!is(idx, GGML_OP_CONT, 2) || idx->type != GGML_TYPE_I32 || idx->ne[1] != B || ggml_nelements(idx) != idx->ne[0] * B) return false;
    const int64_t k = idx->ne[0];
    const ggml_tensor * vw = idx->src[0];
    if (!is(vw, GGML_OP_VIEW, 1) || !is(vw->src[0], GGML_OP_ARGSORT, 1) || vw->data != vw->src[0]->data || vw->ne[0] != k || vw->ne[1] != B) return false;
    const ggml_tensor * srt = vw->src[0], * pr = srt->src[0];
    if (srt->op_params[0] != GGML_SORT_ORDER_DESC || !is(pr, GGML_OP_SOFT_MAX, 2) || pr->src[1] != NULL) return false;
    if (ggml_get_op_params_f32(pr, 0) != 1.0f || ggml_get_op_params_f32(pr, 1) != 0.0f) return false;
    const int64_t n = pr->ne[0];
    if (pr->ne[1] != B || ggml_nelements(pr) != n * B || vw->nb[1] != (size_t) n * 4) return false;
    if (n > SAMPLE_MAX_N || k > SAMPLE_MAX_K || k < 1 || k > n) return false;
    const ggml_tensor * sc = pr->src[0], * inv = nullptr;
    if (is(sc, GGML_OP_SCALE, 1)) { if (ggml_get_op_params_f32(sc, 1) != 0.0f) return false; }
    else if (is(sc, GGML_OP_MUL, 1)) {
        inv = sc->src[1];
        if (!inv || inv->type != GGML_TYPE_F32 || inv->ne[0] != 1 || inv->ne[1] != B || ggml_nelements(inv) != B || !ggml_is_contiguous(inv) || !inv->data) return false;
        if (pos_of(an, inv) >= 0 || inv->view_src) return false;
        for (int j = 0; j < an.g->n_nodes; j++) if (an.g->nodes[j]->view_src == inv) return false;   // (a view of it: something may write through it)
    } else return false;
    const ggml_tensor * logits = sc->src[0];
    if (logits->type != GGML_TYPE_F32 || !ggml_is_contiguous(logits) || ggml_nelements(logits) != n * B || logits->ne[0] != n || !logits->data) return false;
    members.insert(members.end(), { pos_of(an, idx), pos_of(an, vw), pos_of(an, srt), pos_of(an, pr), pos_of(an, sc) });
    // the argmax side: reshape(argmax(div(reshape(get_rows(cont(permute(reshape(p))), idx)), noise)))
    const ggml_tensor * am = through(out->src[1], false);
    if (!is(am, GGML_OP_ARGMAX, 1) || ggml_nelements(am) != B) return false;
    const ggml_tensor * q = am->src[0];
    if (!is(q, GGML_OP_DIV, 1) || q->view_src || q->ne[0] != k || q->ne[1] != B || ggml_nelements(q) != k * B) return false;
    const ggml_tensor * noise = q->src[1];
    if (noise->type != GGML_TYPE_F32 || noise->ne[0] != k || ggml_nelements(noise) != k * B || !ggml_is_contiguous(noise) || !noise->data || pos_of(an, noise) >= 0) return false;
    members.push_back(pos_of(an, am)); members.push_back(pos_of(an, q));
    const ggml_tensor * picked = through(q->src[0], false);
    if (!is(picked, GGML_OP_GET_ROWS, 1) || picked->src[1] != idx || picked->ne[0] != 1) return false;
    members.push_back(pos_of(an, picked));
    const ggml_tensor * c1 = picked->src[0];
    if (!is(c1, GGML_OP_CONT, 1)) return false;
    members.push_back(pos_of(an, c1));
    if (through(c1->src[0], true) != pr) return false;
    for (int m : members) if (m < 0) return false;
    a.logits = (const float *) logits->data; a.n = (int) n; a.k = (int) k; a.B = (int) B;
    a.scale = inv ? 0.f : ggml_get_op_params_f32(sc, 0); a.inv_temp = inv ? (const float *) inv->data : nullptr;
    a.noise = (const float *) noise->data; a.out = (int32_t *) out->data; a.out2 = nullptr;
    // a copy of the B tokens into an I32 vector (the chained Depth graph's token rows): written by the same launch
    for (int j = pos + 1; j < an.g->n_nodes; j++) {
        const ggml_tensor * cp = an.g->nodes[j];
        if (cp->op != GGML_OP_CPY || cp->type != GGML_TYPE_I32 || ggml_nelements(cp) != B || !ggml_is_contiguous(cp) || !cp->data || an.skip[(size_t) j]) continue;
        const ggml_tensor * src = cp->src[0];
        std::vector<int> between;
        while (src != out && src->op == GGML_OP_RESHAPE && pos_of(an, src) >= 0 && uses_of(an, src) == 1) { between.push_back(pos_of(an, src)); src = src->src[0]; }
        if (src != out || !ggml_is_contiguous(cp->src[0])) continue;
        a.out2 = (int32_t *) cp->data; members.push_back(j); members.insert(members.end(), between.begin(), between.end());
        break;
    }
    return true;
}

// H3. the extra heads of a B-column stt step (moshi_hot.cpp build_temporal_graph): for every head k
//    cpy(soft_max(mul_mat(W_k, x)), view k of heads_out)
// with one contiguous F32 x = [K, .., B] (B >= 2 columns of K values) for all heads, W_k dense block-quantised [K, M] rows of one type, K % 256 == 0,
// K <= 16384, M <= HEADS_MAX_M, a plain soft_max (no mask, scale 1), and destinations of M x B floats whose columns are one stride apart and whose rows
// do not overlap. Matched at the first head's mul_mat; claims every such triple over the same x (at most HEADS_MAX) and is emitted where the last
// copy stood. Neither the products nor the soft_max results may have another reader, and nothing else in the graph may touch the destination tensor.
// Anything else (float weights, M > 16) is left to the plain nodes.
struct heads_group : group { heads_streams_args a; };
static bool match_heads_streams(const analysis & an, int pos, heads_group & grp) {
    heads_streams_args & a = grp.a; std::vector<int> & members = grp.members; int & emit_pos = grp.emit_pos;
    const ggml_tensor * mm0 = an.g->nodes[pos];
    if (mm0->op != GGML_OP_MUL_MAT) return false;
    const ggml_tensor * x = mm0->src[1], * w0 = mm0->src[0];
    if (!is_qblock(w0->type) || x->type != GGML_TYPE_F32 || !ggml_is_contiguous(x) || !x->data) return false;
    const int64_t K = w0->ne[0], M = w0->ne[1];
    if (K % 256 != 0 || K > 16384 || M < 1 || M > HEADS_MAX_M || x->ne[0] != K) return false;
    const int64_t B = ggml_nelements(x) / K;
    if (B < 2) return false;
    memset(&a, 0, sizeof(a));
    members.clear();
    const ggml_tensor * root = nullptr;
    int n = 0;
    emit_pos = -1;
    for (int i = pos; i < an.g->n_nodes && n < HEADS_MAX; i++) {
        const ggml_tensor * mm = an.g->nodes[i];
        if (an.skip[(size_t) i] || mm->op != GGML_OP_MUL_MAT || mm->src[1] != x) continue;
        const ggml_tensor * w = mm->src[0];
        if (w->type != w0->type || w->ne[0] != K || w->ne[1] != M || !dense_rows(w) || w->nb[1] != w0->nb[1] || !w->data || ((uintptr_t) w->data & 15) || (w->nb[1] & 15)) continue;
        if (mm->type != GGML_TYPE_F32 || mm->view_src || mm->ne[0] != M || ggml_nelements(mm) != M * B || !ggml_is_contiguous(mm) || uses_of(an, mm) != 1) continue;
        const ggml_tensor * sm = sole_consumer(an, mm);
        if (!sm || sm->op != GGML_OP_SOFT_MAX || sm->src[0] != mm || sm->src[1] != NULL || sm->view_src || uses_of(an, sm) != 1) continue;
        if (ggml_get_op_params_f32(sm, 0) != 1.0f || ggml_get_op_params_f32(sm, 1) != 0.0f) continue;
        const ggml_tensor * cp = sole_consumer(an, sm);
        if (!cp || cp->op != GGML_OP_CPY || cp->src[0] != sm || cp->type != GGML_TYPE_F32 || !cp->data || cp->ne[0] != M || ggml_nelements(cp) != M * B || cp->nb[0] != 4) continue;
        const int psm = pos_of(an, sm), pcp = pos_of(an, cp);
        if (psm < 0 || pcp < 0 || an.skip[(size_t) psm] || an.skip[(size_t) pcp]) continue;
        // the one dimension of the destination that counts the columns
        int bd = -1;
        for (int d = 1; d < 4; d++) if (cp->ne[d] == B) bd = bd < 0 ? d : 4;
        if (bd < 1 || bd > 3 || cp->nb[bd] % 4 != 0 || (int64_t) cp->nb[bd] < M * 4) continue;
        const ggml_tensor * rt = cp->view_src ? cp->view_src : cp;
        if (n == 0) { root = rt; a.out_bs = (int64_t) cp->nb[bd] / 4; }
        else if (rt != root || (int64_t) cp->nb[bd] / 4 != a.out_bs) continue;
        a.w[n] = (const char *) w->data; a.out[n] = (float *) cp->data;
        n++;
        members.insert(members.end(), { i, psm, pcp });
        if (is_view_op(cp->src[1]->op) && pos_of(an, cp->src[1]) >= 0) members.push_back(pos_of(an, cp->src[1]));   // (the destination view: a layout node, no launch)
        if (pcp > emit_pos) emit_pos = pcp;
    }
    if (n == 0 || (const ggml_tensor *) an.g->nodes[members[0]] != mm0) return false;
    // every head's M values of a column lie inside one column period of the destination and no two heads' rows overlap: no two stores of the launch meet
    float * lo = a.out[0];
    for (int k = 1; k < n; k++) if (a.out[k] < lo) lo = a.out[k];
    for (int k = 0; k < n; k++) {
        if (a.out[k] - lo + M > a.out_bs) return false;
        for (int j = 0; j < k; j++) if (a.out[k] - a.out[j] < M && a.out[j] - a.out[k] < M) return false;
    }
    // nothing but the claimed copies touches the destination tensor (a reader between two copies would see some heads only once they move to one launch)
    for (int i = 0; i < an.g->n_nodes; i++) {
        if (std::find(members.begin(), members.end(), i) != members.end()) continue;
        const ggml_tensor * nd = an.g->nodes[i];
        if (nd == root || nd->view_src == root) return false;
        for (int s = 0; s < GGML_MAX_SRC; s++) if (nd->src[s] && (nd->src[s] == root || nd->src[s]->view_src == root)) return false;
    }
    // x must be complete before the first claimed product and is not rewritten before the launch: x is a node (or a leaf) read in place; a writer
    // through an alias between the first product and the emit position would change what the later position reads
    for (int i = pos + 1; i < emit_pos; i++) if (std::find(members.begin(), members.end(), i) == members.end() && writes_through_alias(an.g->nodes[i])) return false;
    a.row_bytes = (int64_t) w0->nb[1]; a.wtype = (int) w0->type; a.K = (int) K; a.M = (int) M; a.n_heads = n; a.B = (int) B;
    a.x = (const float *) x->data; a.x_cs = K;
    return true;
}

// ---- plan construction --------------------------------------------------------------------------------------
// Kernels whose workgroups wait for each other inside a launch (persistent chains, the fused attention + out_proj launch) need their WHOLE grid resident.
// Two such launches from two streams of one device could interleave their dispatch and each keep the other's workgroups off the compute units, so only ONE
// context per device plans them: the first that asks (the LM stream; the codec stream's graphs have no such runs today). Released with the context.
static hip_ctx * g_spin_owner[64];
// (asked only when a plan is about to CONTAIN such a launch: a context that never plans one never claims the device)
static bool is_stream_context(const hip_ctx * c) { for (const hip_ctx * o : stream_contexts()) if (o == c) return true; return false; }
static bool spin_kernels_allowed(hip_ctx * c) {
    if (c->device < 0 || c->device >= 64) return false;
    // An ADDITIONAL command stream (ggml_backend_mi355x_init_stream: the codec stream of the two-stream frame loop) never claims the device: its graphs are the
    // first a frame submits (the encode half), and a claim from there would take the persistent launches away from the LM stream they were built for.
    if (is_stream_context(c)) return false;
    if (!g_spin_owner[c->device]) g_spin_owner[c->device] = c;
    return g_spin_owner[c->device] == c;
}
static bool spin_kernels_possible(const hip_ctx * c) { return c->device >= 0 && c->device < 64 && !is_stream_context(c) && (!g_spin_owner[c->device] || g_spin_owner[c->device] == c); }

// What the passes of build_plan share.
struct planner {
    hip_ctx * c; plan_t * p; ggml_cgraph * g;
    bool keep, fuse;   // keep: the plan is cached or profiled, not launched once and freed; fuse: backend flag 1 is not set
    emitter em;
    analysis an;
    std::map<int, std::vector<pstep>> at_pos;   // fused groups, keyed by the position at which they are emitted
    std::vector<attn_group> attn_groups;        // pass_attention's groups: emitted after pass_matvecs, which absorbs some (emit_pos = -1)
    std::unordered_map<const void *, float *> paired_gate;   // storage of a linear_in output h (never materialised) -> g = silu(h_l) * h_r
};

// THE CLAIM RULE. A group takes its nodes only if every member is a node of the graph (no negative position) and none is claimed already - `self`, the
// node a pass stands on, excepted. Then every member is marked: no later pass matches it, no generic launch is emitted for it.
static bool claimable(const planner & pl, const std::vector<int> & members, int self = -1) {
    for (int m : members) if (m < 0 || (m != self && pl.an.skip[(size_t) m])) return false;
    return true;
}
static bool claim(planner & pl, const std::vector<int> & members, int self = -1) {
    if (!claimable(pl, members, self)) return false;
    for (int m : members) pl.an.skip[(size_t) m] = 1;
    return true;
}
// ... and counted as fused nodes, which every pass but the mat-vec pass does with all its members. Where a pass had no check of its own before this
// rule, the line at its claim says why the rule never refuses there; where its check only lacked `m < 0` (attention, codec convolutions, scalar gathers,
// both samplers, cross-attention, batched mat-muls) it read an.skip[m], so a negative member was an out-of-bounds read already: no matcher returns one.
static bool claim_group(planner & pl, const group & grp, int self = -1) {
    if (!claim(pl, grp.members, self)) return false;
    pl.p->n_fused += (int) grp.members.size();
    return true;
}

// What the run-packers share (pass_cross_attention_blocks, pass_column_attention_rows, merge_column_attention_blocks): groups may share a launch emitted
// at the last of them only if nothing but layout nodes and members of `inside` stands strictly between positions lo and hi ...
static bool clean_between(const planner & pl, int lo, int hi, const std::set<int> & inside) {
    for (int i = lo + 1; i < hi; i++) if (!is_view_op(pl.g->nodes[i]->op) && !inside.count(i)) return false;
    return true;
}
// ... and, for attention groups, only if they agree on everything a launch holds once for all its jobs
static bool same_attention_shape(const attn_args & a, const attn_args & b) {
    return b.H == a.H && b.D == a.D && b.C == a.C && b.scale == a.scale && b.out_ts == a.out_ts && (b.rot != nullptr) == (a.rot != nullptr) &&
           b.q_hs == a.q_hs && b.k_hs == a.k_hs && b.v_hs == a.v_hs && b.k_nb1 == a.k_nb1 && b.k_nb2 == a.k_nb2 && b.v_nb1 == a.v_nb1 && b.v_nb2 == a.v_nb2;
}

// the extra heads of a B-column stt step: every head's mul_mat -> soft_max -> cpy in one launch
static void pass_heads_streams(planner & pl) {
    static const bool no_heads = getenv("MI355X_NO_HEADS_FUSION") != nullptr;
    for (int i = 0; i < pl.g->n_nodes && !no_heads; i++) {
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_MUL_MAT) continue;
        heads_group grp;
        // (claim: the first pass; the matcher tests an.skip for the triples and declines a destination that a non-member touches, so the one member it
        // does not test, the destination view, is in no earlier group of this pass either)
        if (!match_heads_streams(pl.an, i, grp) || !claim_group(pl, grp)) continue;
        const heads_streams_args ha = grp.a;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_heads_streams(s, ha); });
    }
}

// slot snapshots: the K / V ring copies of a fork, a save or a load (moshi_hot.cpp state_graph) - one launch for the whole run
static void pass_ring_copies(planner & pl) {
    for (int i = 0; i < pl.g->n_nodes; i++) {
        ring_copy_group grp;
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_CPY || !match_ring_copies(pl.an, i, grp)) continue;
        if (!claim_group(pl, grp)) continue;   // (claim: every member is a position the matcher's own loop stood on and tested an.skip for)
        const ring_copy_args ra = grp.a; const int cus = pl.c->usable_cus;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_ring_copy(s, ra, cus); });
        pl.p->n_ring_copy_launches++; pl.p->n_ring_copy_jobs += ra.n_jobs;
    }
}

// codec slot snapshots: the conv-state column copies of a fork, a save or a load (moshi_hot.cpp state_graph) - one launch for the whole run
static void pass_state_copies(planner & pl) {
    for (int i = 0; i < pl.g->n_nodes; i++) {
        state_copy_group grp;
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_CPY || !match_state_copies(pl.an, i, grp)) continue;
        if (!claim_group(pl, grp)) continue;   // (claim: every member is a position the matcher's own loop stood on and tested an.skip for)
        const state_copy_args sa = grp.a;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_state_copy(s, sa); });
        pl.p->n_state_copy_launches++; pl.p->n_state_copy_jobs += sa.n_jobs;
    }
}

// attention blocks (they swallow set_rows / soft_max / two mul_mats): collected here, emitted after the mat-vec pass, which may absorb a short-ring
// attention into the projection that consumes it
static void pass_attention(planner & pl) {
    for (int i = 0; i < pl.g->n_nodes; i++) {
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_SOFT_MAX) continue;
        attn_group grp;
        if (!match_attention(pl.an, i, grp) && !match_attention_streams(pl.an, i, grp) && !match_attention_codec_slots(pl.an, i, grp)) continue;
        if (claim_group(pl, grp)) pl.attn_groups.push_back(grp);
    }
    // mask copies that every consumer now bypasses (NOT the claim rule: the copy is no matcher's member, and it is marked and counted as it always was,
    // whatever claimed it before)
    std::map<const ggml_tensor *, int> bypass;
    for (auto & ag : pl.attn_groups) if (ag.mask_node) bypass[ag.mask_node]++;
    for (auto & kv : bypass) if (uses_of(pl.an, kv.first) == kv.second) { pl.an.skip[(size_t) pos_of(pl.an, kv.first)] = 1; pl.p->n_fused++; }
}

// codec convolutions
static void pass_codec_convs(planner & pl) {
    for (int i = 0; i < pl.g->n_nodes; i++) {
        if (pl.an.skip[(size_t) i]) continue;
        step_group grp;
        bool convtr_columns = false, vq_columns = false;
        const enum ggml_op op = pl.g->nodes[i]->op;
        if (op == GGML_OP_MUL_MAT) { if (!match_conv(pl.an, i, grp, pl.em) && !match_conv_columns(pl.an, i, grp)) continue; }
        else if (op == GGML_OP_CONV_TRANSPOSE_1D) {
            if (match_convtr_columns(pl.an, i, grp, pl.em)) convtr_columns = true;
            else if (!match_convtr(pl.an, i, grp, pl.em)) continue;
        }
        else if (op == GGML_OP_ARGMAX) {
            if (!match_vq_level(pl.an, i, grp, pl.em)) {
                if ((pl.c->flags & 8192) || !match_vq_level_columns(pl.an, i, grp, pl.em)) continue;
                vq_columns = true;
            }
        }
        else if (op == GGML_OP_CONCAT) { if (!match_dw_convtr(pl.an, i, grp)) continue; }
        else continue;
        if (!claim_group(pl, grp)) continue;
        if (convtr_columns) pl.p->n_convtr_column_groups++;
        if (vq_columns) pl.p->n_vq_column_levels++;
        for (auto & f : grp.steps) {
            pl.at_pos[grp.emit_pos].push_back(f);
            if (grp.has_vq) { pl.p->vq_copies.emplace_back(new vq_level_args(grp.vq)); pl.at_pos[grp.emit_pos].back().vq = pl.p->vq_copies.back().get(); }
        }
    }
}

// scalar gathers (top-most node first, so it claims the whole tree)
static void pass_scalar_gathers(planner & pl) {
    for (int i = pl.g->n_nodes - 1; i >= 0; i--) {
        if (pl.an.skip[(size_t) i] || !(pl.g->nodes[i]->op == GGML_OP_CPY || pl.g->nodes[i]->op == GGML_OP_CONCAT)) continue;
        step_group grp;
        const int n_cols = match_code_gather(pl.an, i, !(pl.c->flags & 8192), grp);
        if (n_cols < 0 || !claim_group(pl, grp)) continue;
        pl.p->n_code_gather_columns += n_cols;
        for (auto & f : grp.steps) pl.at_pos[grp.emit_pos].push_back(f);
    }
}

static bool no_sampler_fusion() { static const bool off = getenv("MI355X_NO_SAMPLER_FUSION") != nullptr; return off; }
static bool is_sampler_top(const ggml_tensor * n) { return n->op == GGML_OP_GET_ROWS && n->type == GGML_TYPE_I32; }

// top-k samplers (temp > 0)
static void pass_samplers(planner & pl) {
    for (int i = pl.g->n_nodes - 1; i >= 0 && !no_sampler_fusion(); i--) {
        if (pl.an.skip[(size_t) i] || !is_sampler_top(pl.g->nodes[i])) continue;
        step_group grp;
        if (!match_sampler(pl.an, i, grp) || !claim_group(pl, grp)) continue;
        // (a step of its own that a step program may take in: the Depth transformer's samplers sit between its steps' mat-vecs, mv_args::special = 3)
        pl.p->sampler_copies.emplace_back(new sample_args(grp.smp));
        for (auto & f : grp.steps) pl.at_pos[grp.emit_pos].push_back(pstep::special_step(f, 3, nullptr, nullptr, pl.p->sampler_copies.back().get()));
    }
}

// the B-column form of the same samplers (B-column LM steps)
static void pass_sampler_streams(planner & pl) {
    for (int i = pl.g->n_nodes - 1; i >= 0 && !no_sampler_fusion(); i--) {
        if (pl.an.skip[(size_t) i] || !is_sampler_top(pl.g->nodes[i])) continue;
        sampler_streams_group grp;
        if (!match_sampler_streams(pl.an, i, grp) || grp.a.B > pl.c->max_columns || !claim_group(pl, grp)) continue;
        const sample_streams_args sa = grp.a;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_sample_topk_streams(s, sa); });
    }
}

// cross-attention over cached conditions (tts)
static void pass_cross_attention(planner & pl) {
    static const bool no_xattn = getenv("MI355X_NO_CROSS_ATTN_FUSION") != nullptr;
    for (int i = 0; i < pl.g->n_nodes && !no_xattn; i++) {
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_CONT) continue;
        xattn_group grp;
        if (!match_cross_attention(pl.an, i, grp) || !claim_group(pl, grp)) continue;
        const xattn_args xa = grp.a;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_cross_attn(s, xa); });
    }
}

// the cross-attention of a replay pass (tts slots): the run of per-job sequences of one layer - consecutive jobs of one shape with nothing but layout
// nodes and their own members between their copies - as ONE k_cross_attn_blocks launch, emitted where the last of them stood (every job's inputs, the
// layer's query projection and the cached states, are older than the first job; its output rows are read after the last). A run of more than
// XATTN_BLOCKS_MAX jobs takes a further launch.
static void pass_cross_attention_blocks(planner & pl) {
    static const bool no_xattn = getenv("MI355X_NO_CROSS_ATTN_FUSION") != nullptr;
    if (no_xattn) return;
    xattn_blocks_args ba;
    memset(&ba, 0, sizeof(ba));
    int hi = -1;   // emit position of the launch being filled (ba.n_jobs > 0)
    auto flush = [&]() {
        if (!ba.n_jobs) return;
        const xattn_blocks_args la = ba;
        pl.at_pos[hi].push_back([=](hipStream_t s) { k_cross_attn_blocks(s, la); });
        pl.p->n_cross_block_launches++; pl.p->n_cross_block_jobs += la.n_jobs;
        ba.n_jobs = 0;
    };
    for (int i = 0; i < pl.g->n_nodes; i++) {
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_CPY) continue;
        xattn_job_group grp;
        if (!match_cross_attention_job(pl.an, i, grp) || !claimable(pl, grp.members)) continue;
        if (ba.n_jobs) {
            const xattn_args & a = ba.a, & b = grp.a;
            bool joins = ba.n_jobs < XATTN_BLOCKS_MAX && b.H == a.H && b.D == a.D && b.Tc == a.Tc && b.scale == a.scale && b.k_nb1 == a.k_nb1 && b.k_nb2 == a.k_nb2 &&
                         b.v_nb1 == a.v_nb1 && b.v_nb2 == a.v_nb2 && grp.q_rs == ba.q_rs && grp.out_rs == ba.out_rs;
            if (!joins || !clean_between(pl, hi, i, std::set<int>(grp.members.begin(), grp.members.end()))) flush();
        }
        claim_group(pl, grp);
        if (!ba.n_jobs) { ba.a = grp.a; ba.q_rs = grp.q_rs; ba.out_rs = grp.out_rs; }
        ba.job[ba.n_jobs++] = grp.job;
        hi = grp.emit_pos;
    }
    flush();
}

// one embedding row through a small Q8_0 projection (tts: low-rank Depth embeddings)
static void pass_lowrank_embed(planner & pl) {
    static const bool no_lowrank = getenv("MI355X_NO_LOWRANK_FUSION") != nullptr;
    for (int i = 0; i < pl.g->n_nodes && !no_lowrank; i++) {
        lowrank_group grp;
        if (pl.an.skip[(size_t) i] || !match_lowrank_embed(pl.an, i, grp)) continue;
        if (!claim_group(pl, grp)) continue;   // (claim: the matcher tests position and an.skip of the get_rows and of the cast; the mul_mat is node i)
        const lowrank_embed_args la = grp.a;
        pl.p->lowrank_copies.emplace_back(new lowrank_embed_args(la));
        pl.at_pos[grp.emit_pos].push_back(pstep::special_step([=](hipStream_t s) { k_lowrank_embed(s, la); }, 2, nullptr, pl.p->lowrank_copies.back().get()));
    }
}

// the input of a persona pass: the whole concat chain with its embedding sums and row gathers as one launch (top-most concat first)
static void pass_pass_inputs(planner & pl) {
    if (pl.c->flags & 4096) return;   // (the chain stays its plain nodes: an embedding-sum launch per token piece, a row gather per voice piece, the concat copies)
    for (int i = pl.g->n_nodes - 1; i >= 0; i--) {
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_CONCAT) continue;
        pass_input_group grp;
        if (!match_pass_input(pl.an, i, grp) || !claim_group(pl, grp)) continue;   // (claim: the matcher tests position and an.skip of every concat and piece; a sum's terms as pass_embed_sums)
        const pass_input_args a = grp.a;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_pass_input(s, a); });
        pl.p->n_pass_input_launches++; pl.p->n_pass_input_rows += a.B;
    }
}

// embedding sums (top-most add first)
static void pass_embed_sums(planner & pl) {
    for (int i = pl.g->n_nodes - 1; i >= 0; i--) {
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_ADD) continue;
        embed_group grp;
        if (!match_embed_sum(pl.an, i, grp) || !claim_group(pl, grp)) continue;   // (a term that is no node of the graph: a negative member, refused)
        const embed_sum_args a = grp.a;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_embed_sum(s, a); });
    }
}

// a run of cpy(cont(window of a table), row r of dst) for r = 0, 1, .. (stream slots: the B mask rows, moshi_hot.cpp transformer_graph_step_slots):
// one launch for all rows instead of one per row
static void pass_row_copies(planner & pl) {
    for (int i = 0; i < pl.g->n_nodes; i++) {
        row_copy_group grp;
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_CONT || !match_row_copies(pl.an, i, grp)) continue;
        if (!claim_group(pl, grp)) continue;   // (claim: every member is a position the matcher's own loop stood on and tested an.skip for)
        const copy_rows_args ra = grp.a;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_copy_rows(s, ra); });
    }
}

// cpy(cont(x), dst) that the row-copy pass left: the strided source goes straight into dst
static void pass_cpy_of_cont(planner & pl) {
    for (int i = 0; i < pl.g->n_nodes; i++) {
        cpy_fold_group grp;
        if (pl.an.skip[(size_t) i] || !match_cpy_of_cont(pl.an, i, grp)) continue;
        if (!claim_group(pl, grp)) continue;   // (claim: the matcher tests position and an.skip of the cont; the cpy is node i)
        const tdesc d = grp.d, x = grp.x;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_cpy(s, d, x); });
    }
}

// timestep table of add(a, b): one launch
static void pass_timestep_of_add(planner & pl) {
    for (int i = 0; i < pl.g->n_nodes; i++) {
        timestep_group grp;
        if (pl.an.skip[(size_t) i] || !match_timestep_of_add(pl.an, i, grp)) continue;
        if (!claim_group(pl, grp)) continue;   // (claim: the matcher tests position and an.skip of the add; the timestep_embedding is node i)
        const tdesc d = grp.d, tx = grp.x;
        const float * yp = grp.y; const int yn = grp.yn, dim = grp.dim, mp = grp.max_period;
        pstep st([=](hipStream_t s) { k_timestep_embedding(s, d, tx, dim, mp, yp, yn); });
        st.hoist_dst = grp.hoist_dst; st.hoist_bytes = grp.hoist_bytes;
        pl.at_pos[grp.emit_pos].push_back(std::move(st));
    }
}

// ---- the mat-vec pass: four rewrites of one claimed projection `a`, applied in this order ----
// greedy sampling (sampling.h:57-63) as the projection's epilogue: argmax of the logits, optionally copied into the token buffer
static void fold_argmax_epilogue(planner & pl, const mv_group & grp, mv_args & a) {
    static const bool no_argmax_epilogue = getenv("MI355X_NO_ARGMAX_EPILOGUE") != nullptr;
    if (!is_qblock((enum ggml_type) a.wtype) || a.ncols != 1 || no_argmax_epilogue) return;
    const analysis & an = pl.an; const ggml_cgraph * g = pl.g;
    const ggml_tensor * ynode = g->nodes[grp.emit_pos];
    const ggml_tensor * am = nullptr;
    int n_am = 0;
    for (int j = grp.emit_pos + 1; j < g->n_nodes; j++) if (g->nodes[j]->op == GGML_OP_ARGMAX && g->nodes[j]->src[0] == ynode) { am = g->nodes[j]; n_am++; }
    if (!am || n_am != 1 || (float *) ynode->data != a.y || ggml_nelements(ynode) != a.M || !am->data || !claim(pl, { pos_of(an, am) })) return;
    a.argmax_out[0] = (int32_t *) am->data;
    // a copy of the token into an I32 slot
    const ggml_tensor * cp = nullptr;
    for (int j = pos_of(an, am) + 1; j < g->n_nodes; j++)
        if (g->nodes[j]->op == GGML_OP_CPY && g->nodes[j]->src[0] == am && g->nodes[j]->type == GGML_TYPE_I32 && ggml_nelements(g->nodes[j]) == 1) { cp = g->nodes[j]; break; }
    if (cp && claim(pl, { pos_of(an, cp) })) a.argmax_out[1] = (int32_t *) cp->data;
    unsigned * tk = (unsigned *) pl.em.ws(256 + 2 * 4 * 8192);   // arrival counter | per-workgroup argmax candidates (value, index)
    HIP_CHECK(hipMemsetAsync(tk, 0, 256, pl.c->stream));
    a.ticket = tk;
    pl.p->n_fused += 1 + (cp ? 1 : 0);
}

// x is the output of a single-token attention over a short ring (Depth transformer): recompute it in every workgroup of this projection
// instead of launching it on its own (16 heads x 8 slots is ~nothing)
static void fold_short_ring_attention(planner & pl, const mv_group & grp, mv_args & a) {
    static const bool no_attn_prologue = getenv("MI355X_NO_ATTN_PROLOGUE") != nullptr;
    if (a.prologue != MV_PLAIN || !is_qblock((enum ggml_type) a.wtype) || a.ncols != 1 || no_attn_prologue) return;
    for (auto & ag : pl.attn_groups) {
        const attn_args & at = ag.a;
        if (ag.emit_pos < 0 || ag.B > 1 || ag.column || (const float *) at.out != a.x || at.T != 1 || at.D != 64 || at.C > 8 || (int64_t) at.H * at.D != a.K) continue;
        if (a.K != 1024 || at.H != 16 || ag.emit_pos > grp.emit_pos || uses_of(pl.an, pl.g->nodes[ag.emit_pos]) != 1) continue;
        pl.p->attn_copies.emplace_back(new attn_args(at));   // owned by the plan, passed by value at launch
        a.prologue = MV_ATTN;
        a.attn = pl.p->attn_copies.back().get();
        ag.emit_pos = -1;
        return;
    }
}

// the Temporal layer's in_proj at node i, read by nothing but the layer's single-token attention over a LONG ring: the attention runs as the TAIL of
// the projection's own launch (inproj_attn_kernel) - emitted where the attention stood. True: no launch is to be emitted for the projection itself
static bool merge_inproj_attention(planner & pl, int i, const mv_group & grp, const mv_args & a) {
    hip_ctx * c = pl.c; const ggml_cgraph * g = pl.g;
    if (a.prologue != MV_RMSNORM || a.wtype != GGML_TYPE_Q4_K || a.ncols != 1 || !pl.keep || (c->flags & 512) || grp.emit_pos != i) return false;
    for (auto & ag : pl.attn_groups) {
        const attn_args & at = ag.a;
        if (ag.emit_pos < 0 || ag.B > 1 || ag.column || at.q != a.y || ag.emit_pos < grp.emit_pos) continue;
        if (!k_inproj_attn_supported(a, at, c->usable_cus)) continue;
        // every reader of the projection's output must be inside the attention block
        // (followed through layout-only nodes - a view / reshape / permute / transpose of the output is the output: a reader of such an alias that is
        // not part of the attention block would run before the deferred projection has written anything)
        bool private_y = true;
        std::vector<const ggml_tensor *> aliases { g->nodes[i] };
        for (int j = i + 1; j < g->n_nodes && private_y; j++) {
            const ggml_tensor * nj = g->nodes[j];
            bool reads = false;
            for (int sidx = 0; sidx < GGML_MAX_SRC; sidx++)
                if (nj->src[sidx] && std::find(aliases.begin(), aliases.end(), nj->src[sidx]) != aliases.end()) reads = true;
            if (!reads) continue;
            if (is_layout_op(nj->op)) { aliases.push_back(nj); continue; }
            if (std::find(ag.members.begin(), ag.members.end(), j) == ag.members.end()) private_y = false;
        }
        if (!private_y || !spin_kernels_allowed(c)) continue;
        const mv_args am = a; attn_args aa = at;
        aa.short_tail = k_attn_short_tail_default() && !(c->flags & 2048);
        unsigned * err = c->err_dev;
        const size_t wn = k_inproj_attn_ws_size(a, at);
        void * ws = pl.em.ws(wn);
        HIP_CHECK(hipMemsetAsync(ws, 0, wn, c->stream));
        pl.at_pos[ag.emit_pos].insert(pl.at_pos[ag.emit_pos].begin(), [=](hipStream_t s) { k_inproj_attn(s, am, aa, ws, err); });
        ag.emit_pos = -1;
        pl.p->n_fused += 1; pl.p->n_attn_folded++; c->stats.attention_folds_planned++;
        return true;
    }
    return false;
}

// linear_in of a gated FFN at node i whose only readers are the silu(left) * right pair feeding a long linear_out: let every workgroup take
// matching rows of both halves and write g itself (the [2 F] intermediate and the gate kernel disappear)
static void pair_gate_producer(planner & pl, int i, const mv_group & grp, mv_args & a) {
    // on by default (MI355X_PAIRED_GATE=0 turns it off): the gate kernel it removes (-2.3 us per layer) is mostly paid back by linear_out quantising its 44
    // activation blocks in every workgroup (+1.8 us, profiles/r02_frame_stamps_paired_gate.txt) - neutral while the frame waited for the host between graphs,
    // +1.1 % once the LM graphs run back to back (354.7 -> 358.7 frames/s, profiles/r02_ab_paired_gate_run_ahead.txt)
    static const bool no_pair = getenv("MI355X_PAIRED_GATE") != nullptr && atoi(getenv("MI355X_PAIRED_GATE")) == 0;
    if (no_pair || a.prologue == MV_GATE_SILU || a.ncols != 1 || a.residual != nullptr || a.res_embed.table != nullptr || a.ticket != nullptr ||
        a.M % 2 != 0 || !k_matvec_pair_ok(a.wtype, a.K, a.M / 2) || grp.emit_pos != i) return;
    const analysis & an = pl.an; const ggml_cgraph * g = pl.g;
    const ggml_tensor * h = g->nodes[i];
    const int64_t F = a.M / 2;
    const ggml_tensor * l = nullptr, * r = nullptr;
    int nv = 0;
    for (int j = i + 1; j < g->n_nodes && j < i + 12; j++) {
        const ggml_tensor * v = g->nodes[j];
        if (v->op == GGML_OP_VIEW && v->src[0] == h) { nv++; if (v->data == h->data) l = v; else if ((const char *) v->data == (const char *) h->data + F * 4) r = v; }
    }
    if (!(uses_of(an, h) == 2 && nv == 2 && l && r && ggml_nelements(l) == F && ggml_nelements(r) == F && ggml_is_contiguous(l) && ggml_is_contiguous(r) &&
          uses_of(an, l) == 1 && uses_of(an, r) == 1)) return;
    const ggml_tensor * sl = sole_consumer(an, l), * ml = sole_consumer(an, r);
    if (!(sl && sl->op == GGML_OP_UNARY && sl->op_params[0] == GGML_UNARY_OP_SILU && uses_of(an, sl) == 1 && ml && ml->op == GGML_OP_MUL &&
          ml->src[0] == sl && ml->src[1] == r && uses_of(an, ml) == 1)) return;
    const ggml_tensor * mo = sole_consumer(an, ml);
    // the pairing is decided HERE, for both sides: the consumer's own match is run now and must come out as the gated prologue over this
    // very h with none of its members claimed by another group - otherwise h has to be written and nothing is redirected
    if (!(mo && mo->op == GGML_OP_MUL_MAT && mo->src[1] == ml && is_qblock(mo->src[0]->type) && mo->src[0]->ne[0] == F && F > 4096 &&
          !an.skip[(size_t) pos_of(an, mo)])) return;
    mv_group cg;
    const int mpos = pos_of(an, mo);
    if (!(match_matvec(an, mpos, cg) && cg.a.prologue == MV_GATE_SILU && (const void *) cg.a.x == h->data && cg.a.K == F && cg.a.ncols == 1) ||
        !claimable(pl, cg.members, mpos)) return;
    float * gbuf = (float *) pl.em.ws((size_t) F * 4);
    a.pair_F = F;
    a.y = gbuf;
    pl.paired_gate[h->data] = gbuf;
}

// linear_out of a pair: the producer already wrote g = silu(left) * right - plain activation, quantised in this kernel's prologue. True: taken
static bool take_paired_gate(planner & pl, mv_args & a) {
    if (a.prologue != MV_GATE_SILU || !is_qblock((enum ggml_type) a.wtype) || a.K <= 4096 || !pl.paired_gate.count((const void *) a.x)) return false;
    a.x = pl.paired_gate[(const void *) a.x];
    a.prologue = MV_PLAIN;
    a.x_cs = a.K;
    return true;
}

// long gated rows (no pair): quantise the activation once, in a launch in front of the projection, not once per workgroup
static void prequantise_long_gate(planner & pl, const mv_group & grp, mv_args & a) {
    if (a.prologue != MV_GATE_SILU || !is_qblock((enum ggml_type) a.wtype) || a.K <= 4096) return;
    void * blocks = pl.em.ws((size_t) (a.K / 256) * MV_XBLK_BYTES);
    const float * h = a.x; const int64_t K = a.K;
    const int wt = a.wtype;
    pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_gate_quant_q8k(s, h, K, blocks, wt); });
    a.prologue = MV_PREQ8K;
    a.x = (const float *) blocks;
}

// mat-vecs with prologue / epilogue (and, where several rows ride one product, the batched mat-mul). Its members count as fused only when the launch
// replaces more than the mul_mat itself
static void pass_matvecs(planner & pl) {
    static const bool no_batched_fusion = getenv("MI355X_NO_BATCHED_MM") != nullptr || getenv("MI355X_NO_BATCHED_FUSION") != nullptr;
    size_t paired_consumed = 0;
    for (int i = 0; i < pl.g->n_nodes; i++) {
        if (pl.an.skip[(size_t) i] || pl.g->nodes[i]->op != GGML_OP_MUL_MAT) continue;
        mv_group grp;
        if (!match_matvec(pl.an, i, grp)) {
            bmm_group bg;
            if (!no_batched_fusion && match_batched_mm(pl.an, i, pl.em, bg) && claim_group(pl, bg, i)) { pl.at_pos[bg.emit_pos].push_back(bg.run); pl.p->n_float_batched_mms += bg.float_weights && !bg.float_acc; pl.p->n_float_acc_mms += bg.float_acc; }
            continue;
        }
        if (!claim(pl, grp.members, i)) continue;
        const int n_members = grp.members.size() > 1 ? (int) grp.members.size() : 0;
        mv_args a = grp.a;
        fold_argmax_epilogue(pl, grp, a);
        fold_short_ring_attention(pl, grp, a);
        if (merge_inproj_attention(pl, i, grp, a)) { pl.p->n_fused += n_members; continue; }   // (emitted with the attention)
        pair_gate_producer(pl, i, grp, a);
        if (take_paired_gate(pl, a)) paired_consumed++;
        prequantise_long_gate(pl, grp, a);
        pl.at_pos[grp.emit_pos].push_back(pstep(a));
        pl.p->n_fused += n_members;
    }
    GGML_ASSERT(paired_consumed == pl.paired_gate.size() && "a linear_in was redirected to the paired gate form but its linear_out did not pick the gate vector up");
}

// LayerNorm with weight (and bias) over one row that no mat-vec prologue took
static void pass_norm_affine(planner & pl) {
    for (int i = 0; i < pl.g->n_nodes; i++) {
        norm_affine_group grp;
        if (pl.an.skip[(size_t) i] || !match_norm_affine(pl.an, i, grp)) continue;
        if (!claim_group(pl, grp)) continue;   // (claim: the matcher tests position and an.skip of the mul and of the add; the norm is node i)
        const tdesc a = grp.x; const float eps = grp.eps; const int rms = grp.rms;
        const float * wp = grp.w, * bp = grp.b; float * out = grp.out;
        pl.at_pos[grp.emit_pos].push_back([=](hipStream_t s) { k_norm_affine(s, a, eps, rms, wp, bp, out); });
    }
}

// ---- after the fusion passes ----
// slot prefill past the ring's end: the ring-ordered rows of a pass. Each row is a one-row `column` group; a run of at least two of them, consecutive in
// emit order, on the SAME ring column, of one shape, whose q / k / v / out / mask / rot / index bases advance by constant strides, with nothing but
// layout nodes and their own members between their outputs, is a ROWS JOB: the rows must run in order (row t + 1 attends over the ring row that row t
// wrote). The rows jobs of one layer of one pass (consecutive, different columns, same shape) become ONE k_attn_rows launch - at most ATTN_ROWS_MAX
// jobs per launch, further launches beyond - emitted where the last member stood. THE CLAIM: the groups were claimed by pass_attention; a group this
// pass takes leaves the list of groups to emit (emit_pos = -1) and belongs to one rows job only. A run that cannot be proven regular is declined: it
// stays with merge_column_attention_blocks, which never puts two groups of one ring column into a launch pair - a declined row shares a pair only with
// groups of other columns and the pairs run in node order: correct, only slower. A lone one-row group is a block of one row and stays with the block launches. Runs before merge_column_attention_blocks.
static bool no_attn_rows() { static const bool off = getenv("MI355X_NO_ATTN_ROWS") != nullptr; return off; }
static void pass_column_attention_rows(planner & pl) {
    if (no_attn_rows()) return;
    std::vector<attn_group> & groups = pl.attn_groups;
    std::vector<size_t> order;   // the column groups in emit order (the order their outputs stand in the graph)
    for (size_t i = 0; i < groups.size(); i++) if (groups[i].column && groups[i].emit_pos >= 0 && groups[i].B == 1) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return groups[x].emit_pos < groups[y].emit_pos; });
    auto same_shape = [](const attn_args & a, const attn_args & b) { return b.T == 1 && same_attention_shape(a, b); };   // rows: one-row groups only
    auto stride = [](const void * a, const void * b) { return (int64_t) ((const char *) b - (const char *) a); };
    attn_rows_args ra;
    int launch_hi = -1;           // emit position of the launch being filled (ra.n_jobs > 0)
    std::set<int> rows_inside;    // the members of the rows jobs of that launch
    auto flush = [&]() {
        if (!ra.n_jobs) return;
        const attn_rows_args la = ra;
        unsigned * err = pl.c->err_dev;
        auto & at = pl.at_pos[launch_hi];
        at.insert(at.begin(), [=](hipStream_t s) { k_attn_rows(s, la, err); });
        pl.p->n_attn_row_launches++; pl.p->n_attn_row_jobs += la.n_jobs;
        for (int j = 0; j < la.n_jobs; j++) pl.p->n_attn_row_rows += la.job[j].n;
        ra.n_jobs = 0;
    };
    memset(&ra, 0, sizeof(ra));
    for (size_t oi = 0; oi < order.size(); ) {
        const attn_group & g0 = groups[order[oi]];
        const attn_args & a0 = g0.a;
        size_t oe = oi + 1;
        std::set<int> inside(g0.members.begin(), g0.members.end());
        int hi = g0.emit_pos;
        attn_rows_job jb;
        memset(&jb, 0, sizeof(jb));
        if (a0.T == 1) {
            while (oe < order.size() && oe - oi < 64) {
                const attn_group & gn = groups[order[oe]];
                const attn_args & b = gn.a, & prev = groups[order[oe - 1]].a;
                if (!same_shape(a0, b) || b.kcache != a0.kcache || b.vcache != a0.vcache) break;
                const int64_t d[7] = { stride(prev.q, b.q), stride(prev.k, b.k), stride(prev.v, b.v), stride(prev.mask, b.mask), b.rot ? stride(prev.rot, b.rot) : 0,
                                       stride(prev.index, b.index), stride(prev.out, b.out) };
                if (oe == oi + 1) { jb.q_rs = d[0]; jb.k_rs = d[1]; jb.v_rs = d[2]; jb.mask_rs = d[3]; jb.rot_rs = d[4]; jb.index_rs = d[5]; jb.out_rs = d[6]; }
                else if (d[0] != jb.q_rs || d[1] != jb.k_rs || d[2] != jb.v_rs || d[3] != jb.mask_rs || d[4] != jb.rot_rs || d[5] != jb.index_rs || d[6] != jb.out_rs) break;
                if (d[0] % 4 || d[1] % 4 || d[2] % 4 || d[3] % 4 || d[4] % 4 || d[5] % 4 || d[6] % 4) break;
                std::set<int> both = inside;
                both.insert(gn.members.begin(), gn.members.end());
                if (!clean_between(pl, hi, gn.emit_pos, both)) break;
                inside.swap(both); hi = gn.emit_pos;
                oe++;
            }
        }
        const int n = (int) (oe - oi);
        if (n < 2) { flush(); oi = oe; continue; }   // a block-form job (or a lone row): not this pass's; it also ends the layer's run of rows jobs
        // a further rows job of the same launch: same shape, another column, nothing foreign between the launch so far and this job
        if (ra.n_jobs) {
            bool joins = ra.n_jobs < ATTN_ROWS_MAX && same_shape(ra.a, a0);
            for (int j = 0; j < ra.n_jobs && joins; j++) joins = ra.job[j].kcache != a0.kcache && ra.job[j].vcache != a0.vcache;
            if (joins) {
                std::set<int> both = inside;
                both.insert(rows_inside.begin(), rows_inside.end());
                joins = clean_between(pl, launch_hi, g0.emit_pos, both);
            }
            if (!joins) flush();
        }
        if (!ra.n_jobs) { ra.a = a0; rows_inside.clear(); }
        jb.q = (const char *) a0.q; jb.k = (const char *) a0.k; jb.v = (const char *) a0.v; jb.kcache = a0.kcache; jb.vcache = a0.vcache;
        jb.mask = (const char *) a0.mask; jb.rot = (const char *) a0.rot; jb.index = (const char *) a0.index; jb.out = (char *) a0.out; jb.n = n;
        ra.job[ra.n_jobs++] = jb;
        rows_inside.insert(inside.begin(), inside.end());
        launch_hi = hi;
        for (size_t k = oi; k < oe; k++) groups[order[k]].emit_pos = -1;
        oi = oe;
    }
    flush();
}

// slot prefill: the column groups of one layer of one pass (consecutive groups of one shape with nothing but layout nodes and their own members
// between their outputs) become ONE pair of k_attn_blocks launches, emitted where the last of them stood: a write phase, then an attend phase
static void merge_column_attention_blocks(planner & pl) {
    std::vector<attn_group> & attn_groups = pl.attn_groups;
    for (size_t gi = 0; gi < attn_groups.size(); ) {
        if (!attn_groups[gi].column || attn_groups[gi].emit_pos < 0) { gi++; continue; }
        const attn_args & a0 = attn_groups[gi].a;
        std::set<int> inside(attn_groups[gi].members.begin(), attn_groups[gi].members.end());
        size_t ge = gi + 1;
        int lo = attn_groups[gi].emit_pos, hi = lo;
        // the row strides of q / k / v mean nothing to a one-row job (strided_resolve leaves them 0): the jobs of more than one row must agree on them
        const attn_args * rows = a0.T > 1 ? &a0 : nullptr;
        while (ge < attn_groups.size() && ge - gi < ATTN_BLOCKS_MAX) {
            const attn_group & n = attn_groups[ge];
            const attn_args & b = n.a;
            if (!n.column || n.emit_pos < 0 || !same_attention_shape(a0, b) || (b.T > 1 && rows && (b.q_ts != rows->q_ts || b.k_ts != rows->k_ts || b.v_ts != rows->v_ts))) break;
            // a launch pair never holds two groups of one ring column: it writes every job's rows before any job attends, so a second group of a column
            // (a ring-ordered row after its predecessor, where pass_column_attention_rows is off or has declined the run) must start a launch of its own
            bool column_taken = false;
            for (size_t k = gi; k < ge && !column_taken; k++) column_taken = attn_groups[k].a.kcache == b.kcache || attn_groups[k].a.vcache == b.vcache;
            if (column_taken) break;
            std::set<int> both = inside;
            both.insert(n.members.begin(), n.members.end());
            const int nlo = n.emit_pos < lo ? n.emit_pos : lo, nhi = n.emit_pos > hi ? n.emit_pos : hi;
            if (!clean_between(pl, nlo, nhi, both)) break;
            inside.swap(both); lo = nlo; hi = nhi;
            if (b.T > 1 && !rows) rows = &b;
            ge++;
        }
        attn_blocks_args ba;
        memset(&ba, 0, sizeof(ba));
        ba.a = a0;
        if (rows) { ba.a.q_ts = rows->q_ts; ba.a.k_ts = rows->k_ts; ba.a.v_ts = rows->v_ts; }
        ba.n_jobs = (int) (ge - gi);
        for (size_t k = gi; k < ge; k++) {
            const attn_args & b = attn_groups[k].a;
            ba.job[k - gi] = { b.q, b.k, b.v, b.kcache, b.vcache, b.mask, b.rot, b.index, b.out, b.T };
            attn_groups[k].emit_pos = -1;
        }
        unsigned * err = pl.c->err_dev;
        auto & at = pl.at_pos[hi];
        at.insert(at.begin(), [=](hipStream_t s) { attn_blocks_args b = ba; b.write_only = 0; k_attn_blocks(s, b, err); });
        at.insert(at.begin(), [=](hipStream_t s) { attn_blocks_args b = ba; b.write_only = 1; k_attn_blocks(s, b, err); });
        pl.p->n_attn_block_launches += 2; pl.p->n_attn_block_jobs += ba.n_jobs;
        gi = ge;
    }
}

// the attention groups nothing absorbed, each in FRONT of whatever else is emitted at its position
static void emit_attention_groups(planner & pl) {
    hip_ctx * c = pl.c;
    for (auto & ag : pl.attn_groups) {
        if (ag.emit_pos < 0) continue;
        const attn_args a = ag.a;
        unsigned * err = c->err_dev;
        auto & at = pl.at_pos[ag.emit_pos];
        if (ag.B > 1 && ag.sa.a.T > 1) {   // decoder slots: one launch for every (head, row, column)
            const attn_streams_args sa = ag.sa;
            at.insert(at.begin(), [=](hipStream_t s) { k_attn_codec_slots(s, sa); });
            pl.p->n_codec_attn_launches++;
            continue;
        }
        if (ag.B > 1) {   // lockstep streams: one launch for every (head, stream)
            const attn_streams_args sa = ag.sa;
            at.insert(at.begin(), [=](hipStream_t s) { k_attn_streams(s, sa, err); });
            continue;
        }
        if (a.T > 4) {
            // a block of T > 4 new rows (batched prompt prefill): one workgroup per head and group of 4 rows; first every row's K / V
            // goes into the ring, then all groups attend at once (causality is in the mask rows)
            at.insert(at.begin(), [=](hipStream_t s) {
                attn_args b = a;
                b.n_groups = (a.T + 3) / 4;
                b.write_only = 1; k_attn_decode(s, b, nullptr, err);
                b.write_only = 0; k_attn_decode(s, b, nullptr, err);
            });
            continue;
        }
        void * ws = nullptr;
        if (const size_t n = k_attn_split_resident(a, c->usable_cus) ? k_attn_decode_ws_size(a) : 0) { ws = pl.em.ws(n); HIP_CHECK(hipMemsetAsync(ws, 0, n, c->stream)); }   // sequence numbers start at zero
        if (a.T <= 4 && a.n_groups <= 1 && !ws) {
            pl.p->attn_copies.emplace_back(new attn_args(a));
            at.insert(at.begin(), pstep::special_step([=](hipStream_t s) { k_attn_decode(s, a, ws, err); }, 1, pl.p->attn_copies.back().get(), nullptr));
        } else
            at.insert(at.begin(), [=](hipStream_t s) { k_attn_decode(s, a, ws, err); });
    }
}

static bool dump_plan() { return getenv("MI355X_DUMP_PLAN") != nullptr; }

// the plan's steps in node order: a generic launch for every node nobody claimed, then the groups emitted at that position (MI355X_DUMP_PLAN lists both)
static void lay_out_steps(planner & pl) {
    const bool dump = dump_plan();
    const ggml_cgraph * g = pl.g;
    for (int i = 0; i < g->n_nodes; i++) {
        auto it = pl.at_pos.find(i);
        if (dump) {
            const ggml_tensor * n = g->nodes[i];
            const bool layout = is_layout_op(n->op);
            if (!layout || it != pl.at_pos.end())
                fprintf(stderr, "plan %4d %-18s [%5lld %5lld %4lld %2lld] %s%s%s\n", i, ggml_op_name(n->op), (long long) n->ne[0], (long long) n->ne[1], (long long) n->ne[2],
                        (long long) n->ne[3], pl.an.skip[(size_t) i] ? "fused" : (layout ? "-" : "GENERIC"), it != pl.at_pos.end() ? " <emit group>" : "", n->view_src ? " (alias)" : "");
        }
        if (!pl.an.skip[(size_t) i]) {
            if (g->nodes[i]->op == GGML_OP_SOFT_MAX || g->nodes[i]->op == GGML_OP_SET_ROWS) pl.p->n_generic_attn_nodes++;
            emit_generic(pl.em, g->nodes[i]);
        }
        if (it != pl.at_pos.end()) for (auto & f : it->second) pl.p->steps.push_back(f);
    }
}

// The codec transformers' RoPE table sits between layer 0's in_proj and its attention in node order: moved in front of that in_proj (whose operands it
// does not touch), the whole stack is one run (hip_chain_mimi.h takes it from in_proj 0; otherwise the program starts at layer 0's attention).
static void hoist_rope_tables(planner & pl) {
    plan_t * p = pl.p;
    for (size_t i = 1; i + 1 < p->steps.size(); i++) {
        pstep & h = p->steps[i];
        const pstep & m = p->steps[i - 1];
        if (!h.hoist_dst || !m.is_mv || m.mv.special || m.mv.wtype != GGML_TYPE_F32 || m.mv.ncols != 2 || !p->steps[i + 1].is_mv) continue;
        auto clash = [&](const float * q, int64_t n_floats) { return q && (const char *) q < h.hoist_dst + h.hoist_bytes && h.hoist_dst < (const char *) (q + n_floats); };
        const mv_args & a = m.mv;
        if (clash(a.x, a.x_cs * (a.ncols - 1) + a.K) || clash(a.y, a.y_cs * (a.ncols - 1) + a.M) || clash(a.x_out, a.K * a.ncols) || clash(a.residual, a.r_cs * (a.ncols - 1) + a.M) ||
            clash(a.alpha, a.K) || clash(a.beta, a.K)) continue;
        std::swap(p->steps[i - 1], p->steps[i]);
    }
}

// Persistent chains: a run of consecutive block mat-vecs each of which waits on its predecessor (the chained Depth transformer,
// lm.h:446-553: 26 mat-vecs per step, 8 / 16 steps per graph) becomes ONE launch of the chain engine (hip_chain.hip).
// (only for plans that are kept - cached graphs, profile mode: a one-off plan is launched once and freed at once, a chain's tables would be built,
// uploaded and torn down per compute)
static bool chains_wanted(const planner & pl) {
    return pl.fuse && pl.keep && !(pl.c->flags & 16) && ((pl.c->flags & 32) || k_chain_default_on()) && spin_kernels_possible(pl.c);
}
static void merge_chains(planner & pl) {
    const bool dump = dump_plan();
    hip_ctx * c = pl.c; plan_t * p = pl.p; emitter & em = pl.em;
    std::vector<pstep> merged;
    size_t i = 0;
    while (i < p->steps.size()) {
        if (p->steps[i].vq) {
            // consecutive levels of one RVQ encode stack (vq.h:97-114): one persistent launch with a candidate hand-off per level (hip_chain.hip, vq_chain_kernel)
            size_t e = i;
            std::vector<vq_level_args> lv;
            while (e < p->steps.size() && p->steps[e].vq && lv.size() < 32 && (lv.empty() || ((const void *) p->steps[e].vq->resid == (const void *) lv.back().resid_out && p->steps[e].vq->resid_stride == 4))) {
                lv.push_back(*p->steps[e].vq); e++;
            }
            if (lv.size() >= 2 && k_vq_chain_accept(lv.data(), (int) lv.size(), c->usable_cus) && spin_kernels_allowed(c)) {
                void * ws = em.ws(k_vq_chain_ws_size((int) lv.size()));
                vq_chain_plan * vc = k_vq_chain_create(c->stream, lv.data(), (int) lv.size(), ws, c->err_dev);
                p->vq_chains.push_back(vc);
                p->n_vq_chained += (int) lv.size();
                merged.push_back(pstep([vc](hipStream_t s) { k_vq_chain_launch(s, vc); }));
                if (dump) fprintf(stderr, "plan: %zu consecutive RVQ levels -> one launch\n", lv.size());
                i = e;
                continue;
            }
            merged.push_back(std::move(p->steps[i])); i++; continue;
        }
        if (!p->steps[i].is_mv) { merged.push_back(std::move(p->steps[i])); i++; continue; }
        size_t e = i;
        while (e < p->steps.size() && p->steps[e].is_mv) e++;
        std::vector<mv_args> run;
        for (size_t k = i; k < e; k++) run.push_back(p->steps[k].mv);
        size_t k = 0;
        while (k < run.size()) {
            int len = k_chain_accept(run.data() + k, (int) (run.size() - k), c->usable_cus, !(c->flags & 1024));
            if (len > 0 && !spin_kernels_allowed(c)) len = 0;
            if (len <= 0) {
                merged.push_back(std::move(p->steps[i + k])); k++; continue;
            }
            void * ws = em.ws(k_chain_ws_size(run.data() + k, len, c->usable_cus, !(c->flags & 1024)));
            chain_plan * ch = k_chain_create(c->stream, run.data() + k, len, ws, c->err_dev, c->usable_cus, !(c->flags & 1024));
            p->chains.push_back(ch);
            if (k_chain_is_step_program(ch)) p->n_step_programs++;
            merged.push_back(pstep([ch](hipStream_t s) { k_chain_launch(s, ch); }));
            merged.back().chain = ch;
            p->n_chained += len;
            if (dump) fprintf(stderr, "plan: %d consecutive mat-vecs -> one chain launch (%.1f MB of weights)\n", len, (double) k_chain_weight_bytes(ch) / 1e6);
            k += (size_t) len;
        }
        i = e;
    }
    p->steps.swap(merged);
}

// THE PASS ORDER. A node belongs to the first group that claims it, so the order of this list is part of what a plan is. The reasons on record:
//   pass_heads_streams     before the generic mat-vecs, which would take the heads' mul_mats one by one; first of all, which its claim relies on
//   pass_attention         attention blocks first: they swallow set_rows / soft_max / two mul_mats. Collected before the mat-vec pass and emitted after
//                          it, because that pass may absorb a short-ring attention into the projection that consumes it, or run a long-ring one as
//                          the tail of its in_proj
//   pass_scalar_gathers    bottom-up over the node list: the top-most node first, so it claims the whole tree
//   pass_samplers          bottom-up as well: matched at the sampler's last node
//   pass_sampler_streams   the B-column form of the same samplers, same direction
//   pass_cross_attention_blocks   the per-job cross-attention of a tts replay pass: before the row copies and the mat-vec pass, which would take a job's
//                          copy and its F32 mul_mats one by one
//   pass_pass_inputs       before pass_embed_sums, which would take the sums of a persona pass's token pieces one by one; bottom-up (the top-most concat)
//   pass_embed_sums        bottom-up (a left-deep sum is matched at its last add); before the row copies
//   pass_row_copies        one launch for all rows instead of one per row: before pass_cpy_of_cont, whose pattern every single row is
//   pass_matvecs           after the attention pass (see there); every remaining mul_mat of a supported shape
//   pass_norm_affine       after the mat-vec pass: only a norm that no mat-vec prologue took
//   pass_state_copies      last: it takes only column copies that no other pass wanted, so no plan that existed before it loses a node to it
// (pass_ring_copies, pass_codec_convs, pass_cross_attention, pass_lowrank_embed, pass_cpy_of_cont, pass_timestep_of_add: no reason on record but their place)
static void (* const fusion_passes[])(planner &) = {
    pass_heads_streams, pass_ring_copies, pass_attention, pass_codec_convs, pass_scalar_gathers, pass_samplers, pass_sampler_streams, pass_cross_attention,
    pass_cross_attention_blocks, pass_lowrank_embed, pass_pass_inputs, pass_embed_sums, pass_row_copies, pass_cpy_of_cont, pass_timestep_of_add, pass_matvecs, pass_norm_affine, pass_state_copies,
};

static plan_t * build_plan(hip_ctx * c, ggml_cgraph * g, bool keep = true) {
    planner pl;
    pl.c = c; pl.p = new plan_t; pl.g = g;
    pl.keep = keep; pl.fuse = !(c->flags & 1);
    pl.em.c = c; pl.em.p = pl.p;
    pl.p->n_nodes = g->n_nodes;
    analyse(pl.an, g);
    collect_plan_buffers(pl.p, g);
    if (pl.fuse) for (auto pass : fusion_passes) pass(pl);
    // the attention groups no projection absorbed: the ring-ordered rows of a slot prefill pass as rows launches, its other column groups as launch
    // pairs, the rest one by one
    pass_column_attention_rows(pl);
    merge_column_attention_blocks(pl);
    emit_attention_groups(pl);
    lay_out_steps(pl);
    if (chains_wanted(pl)) {
        hoist_rope_tables(pl);   // (so that the codec stacks are one run of mat-vecs)
        merge_chains(pl);
    }
    return pl.p;
}

static void run_steps(hip_ctx * c, plan_t * p) { for (auto & st : p->steps) st.fn(c->stream); }

// flag 8: launch eagerly with start/stop events on every matvec_q4k_kernel dispatch and accumulate
static void run_steps_profiled(hip_ctx * c, plan_t * p) {
    if (!c->prof.recs) {
        c->prof.capacity = 4096;
        c->prof.recs = new mv_profile::rec[(size_t) c->prof.capacity];
        for (int i = 0; i < c->prof.capacity; i++) { HIP_CHECK(hipEventCreate(&c->prof.recs[i].start)); HIP_CHECK(hipEventCreate(&c->prof.recs[i].stop)); }
    }
    c->prof.used = 0;
    k_matvec_set_profile(&c->prof);
    for (auto & st : p->steps) {
        if (!st.chain) { st.fn(c->stream); continue; }
        // a persistent chain launch: one kernel, timed between two stream events
        if (!c->chain_ev[0]) { HIP_CHECK(hipEventCreate(&c->chain_ev[0])); HIP_CHECK(hipEventCreate(&c->chain_ev[1])); }
        HIP_CHECK(hipStreamSynchronize(c->stream));
        HIP_CHECK(hipEventRecord(c->chain_ev[0], c->stream));
        st.fn(c->stream);
        HIP_CHECK(hipEventRecord(c->chain_ev[1], c->stream));
        HIP_CHECK(hipEventSynchronize(c->chain_ev[1]));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, c->chain_ev[0], c->chain_ev[1]));
        c->prof_chain_seconds += (double) ms * 1e-3; c->prof_chain_launches++; c->prof_chain_bytes += k_chain_weight_bytes(st.chain); c->prof_chain_phases += k_chain_length(st.chain);
    }
    k_matvec_set_profile(nullptr);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < c->prof.used; i++) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, c->prof.recs[i].start, c->prof.recs[i].stop));
        const int v = c->prof.recs[i].variant == 2 ? 2 : c->prof.recs[i].variant ? 1 : 0;
        if (v != 2) {   // the totals are matvec_q4k_kernel's own (what a profiler lists under that name); inproj_attn_kernel is reported as its own variant
            c->prof_seconds += (double) ms * 1e-3;
            c->prof_launches++;
            c->prof_bytes += c->prof.recs[i].bytes;
        }
        c->prof_seconds_v[v] += (double) ms * 1e-3; c->prof_launches_v[v]++; c->prof_bytes_v[v] += c->prof.recs[i].bytes;
    }
}

// the *_in_last_plan counters of ggml_mi355x_stats: what the plan of the graph computed last holds
static void publish_plan_stats(hip_ctx * c, const plan_t * p) {
    c->stats.kernels_in_last_plan = (int64_t) p->steps.size();
    c->stats.nodes_in_last_plan = p->n_nodes;
    c->stats.fused_nodes_in_last_plan = p->n_fused;
    c->stats.chained_matvecs_in_last_plan = p->n_chained; c->stats.chain_step_programs_in_last_plan = p->n_step_programs; c->stats.vq_levels_chained_in_last_plan = p->n_vq_chained;
    c->stats.attn_block_launches_in_last_plan = p->n_attn_block_launches; c->stats.attn_block_jobs_in_last_plan = p->n_attn_block_jobs; c->stats.generic_attention_nodes_in_last_plan = p->n_generic_attn_nodes;
    c->stats.ring_copy_launches_in_last_plan = p->n_ring_copy_launches; c->stats.ring_copy_jobs_in_last_plan = p->n_ring_copy_jobs;
    c->stats.attn_row_launches_in_last_plan = p->n_attn_row_launches; c->stats.attn_row_jobs_in_last_plan = p->n_attn_row_jobs; c->stats.attn_row_rows_in_last_plan = p->n_attn_row_rows;
    c->stats.cross_block_launches_in_last_plan = p->n_cross_block_launches; c->stats.cross_block_jobs_in_last_plan = p->n_cross_block_jobs;
    c->stats.float_batched_mms_in_last_plan = p->n_float_batched_mms;
    c->stats.float_acc_mms_in_last_plan = p->n_float_acc_mms;
    c->stats.pass_input_launches_in_last_plan = p->n_pass_input_launches; c->stats.pass_input_rows_in_last_plan = p->n_pass_input_rows;
    c->stats.convtr_column_groups_in_last_plan = p->n_convtr_column_groups; c->stats.codec_attn_launches_in_last_plan = p->n_codec_attn_launches;
    c->stats.vq_column_levels_in_last_plan = p->n_vq_column_levels; c->stats.code_gather_columns_in_last_plan = p->n_code_gather_columns;
    c->stats.state_copy_launches_in_last_plan = p->n_state_copy_launches; c->stats.state_copy_jobs_in_last_plan = p->n_state_copy_jobs;
}

static enum ggml_status hip_graph_compute(ggml_backend_t backend, struct ggml_cgraph * g) {
    hip_ctx * c = (hip_ctx *) backend->context;
    ctx_init_lazy(c);
    set_device(c);
    flush_uploads(c);
    c->stats.graphs_computed++;
    if (g->n_nodes == 0) return GGML_STATUS_SUCCESS;

    if (c->flags & 8) {
        plan_t * p = build_plan(c, g);
        run_steps_profiled(c, p);
        plan_free(c, p);
        return GGML_STATUS_SUCCESS;
    }
    const bool cacheable = g->n_nodes >= 32;
    if (!cacheable) {
        plan_t * p = build_plan(c, g, false);
        run_steps(c, p);
        publish_plan_stats(c, p);
        plan_free(c, p);   // workspaces return to the pool; reuse is stream-ordered
        return GGML_STATUS_SUCCESS;
    }

    const uint64_t h = graph_hash(g);
    plan_t * p = nullptr;
    auto it = c->plans.find(g);
    if (it != c->plans.end()) {
        if (it->second->hash == h) { p = it->second; if (p->orphan_seq) { p->orphan_seq = 0; collect_plan_buffers(p, g); } }
        else { HIP_CHECK(hipStreamSynchronize(c->stream)); plan_free(c, it->second); c->plans.erase(it); }
    }
    static const bool time_plan = getenv("MI355X_TIME_PLAN") != nullptr;
    const int64_t tp0 = time_plan ? ggml_time_us() : 0;
    bool fresh = false;
    if (!p) {
        p = build_plan(c, g);
        p->hash = h;
        c->plans[g] = p;
        fresh = true;
    }
    const int64_t tp1 = time_plan ? ggml_time_us() : 0;
    if (!fresh && !p->exec && !(c->flags & 2) && !c->no_capture) {
        // second compute of the same graph: it is a cached graph (the per-frame ones), so capture the launch sequence now; replays cost one
        // hipGraphLaunch. One-shot graphs (scratch contexts, prompt prefill chunks) never pay for a capture.
        HIP_CHECK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        run_steps(c, p);
        HIP_CHECK(hipStreamEndCapture(c->stream, &p->graph));
        HIP_CHECK(hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0));
    }
    const int64_t tp2 = time_plan ? ggml_time_us() : 0;
    if (p->exec) { HIP_CHECK(hipGraphLaunch(p->exec, c->stream)); c->stats.graph_replays++; }
    else run_steps(c, p);
    if (time_plan && g->n_nodes > 500)
        fprintf(stderr, "graph %p nodes %d: plan %s %.2f ms, capture %.2f ms, launch %.2f ms (%zu kernels)\n", (void *) g, g->n_nodes, fresh ? "built" : "reused",
                (tp1 - tp0) / 1e3, (tp2 - tp1) / 1e3, (ggml_time_us() - tp2) / 1e3, p->steps.size());
    publish_plan_stats(c, p);
    return GGML_STATUS_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// backend / device / registry objects
// ---------------------------------------------------------------------------------------------------
static const char * hip_backend_name(ggml_backend_t b) { return ((hip_ctx *) b->context)->name.c_str(); }
static void hip_backend_free(ggml_backend_t b) {
    hip_ctx * c = (hip_ctx *) b->context;
    if (c->stream) {
        set_device(c);
        (void) hipStreamSynchronize(c->stream);
        for (auto & kv : c->plans) plan_free(c, kv.second);
        c->plans.clear();
    }
    if (c->device >= 0 && c->device < 64 && g_spin_owner[c->device] == c) g_spin_owner[c->device] = nullptr;   // (its plans are gone)
    c->in_use = false;
    delete b;
}
static void hip_backend_sync(ggml_backend_t b) {
    hip_ctx * c = (hip_ctx *) b->context;
    if (!c->stream) return;
    set_device(c);
    flush_uploads(c);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    deliver_async_gets(c, c->aget_seq);
}
// ggml_backend_tensor_get_async: a copy queued behind the submitted work into a pinned slot; larger reads take the blocking path
static void hip_get_tensor_async(ggml_backend_t b, const struct ggml_tensor * t, void * data, size_t offset, size_t size) {
    hip_ctx * c = (hip_ctx *) b->context;
    if (size > AGET_SLOT_BYTES) { ggml_backend_tensor_get(t, data, offset, size); return; }
    ctx_init_lazy(c);
    set_device(c);
    flush_uploads(c);
    if (c->aget_pending.size() >= AGET_SLOTS) { HIP_CHECK(hipStreamSynchronize(c->stream)); deliver_async_gets(c, c->aget_seq); }
    const uint64_t seq = ++c->aget_seq;
    const int slot = (int) (seq % AGET_SLOTS);
    HIP_CHECK(hipMemcpyAsync(c->aget_pinned + (size_t) slot * AGET_SLOT_BYTES, (const char *) t->data + offset, size, hipMemcpyDeviceToHost, c->stream));
    c->aget_pending.push_back({ data, size, slot, seq });
}
struct hip_event_ctx { hipEvent_t ev; hip_ctx * c; uint64_t seq; };
static void hip_event_sync(ggml_backend_event_t e) {
    hip_event_ctx * h = (hip_event_ctx *) e->context;
    set_device(h->c);
    HIP_CHECK(hipEventSynchronize(h->ev));
    deliver_async_gets(h->c, h->seq);
    check_device_error(h->c);
}
static void hip_event_free(ggml_backend_event_t e) { hip_event_ctx * h = (hip_event_ctx *) e->context; if (h) { (void) hipEventDestroy(h->ev); delete h; } e->context = NULL; }
static void hip_event_record(ggml_backend_t b, ggml_backend_event_t e) {
    hip_ctx * c = (hip_ctx *) b->context;
    ctx_init_lazy(c);
    set_device(c);
    hip_event_ctx * h = (hip_event_ctx *) e->context;
    if (!h) {
        h = new hip_event_ctx;
        HIP_CHECK(hipEventCreateWithFlags(&h->ev, hipEventDisableTiming));
        e->context = h; e->synchronize = hip_event_sync; e->free_context = hip_event_free;
    }
    flush_uploads(c);
    h->c = c; h->seq = c->aget_seq;
    HIP_CHECK(hipEventRecord(h->ev, c->stream));
}
static void hip_event_wait(ggml_backend_t b, ggml_backend_event_t e) {
    hip_ctx * c = (hip_ctx *) b->context;
    hip_event_ctx * h = (hip_event_ctx *) e->context;
    if (!h) return;                      // never recorded: nothing to wait for
    ctx_init_lazy(c);
    set_device(c);
    flush_uploads(c);
    HIP_CHECK(hipStreamWaitEvent(c->stream, h->ev, 0));
}
static bool hip_supports_op(ggml_backend_t, const struct ggml_tensor * op) {
    switch (op->op) {
        case GGML_OP_CPY: case GGML_OP_CONT: case GGML_OP_DUP:
            if (ggml_is_quantized(op->type) || ggml_is_quantized(op->src[0]->type)) {
                if (op->type == op->src[0]->type) return true;
                // load-time (re)quantisation of float rows (src/loader.h:160-187): F32 / F16 / BF16 -> Q8_0 / Q4_0 / Q4_K
                const enum ggml_type st = op->src[0]->type;
                return (st == GGML_TYPE_F32 || st == GGML_TYPE_F16 || st == GGML_TYPE_BF16) &&
                       (op->type == GGML_TYPE_Q8_0 || op->type == GGML_TYPE_Q4_0 || op->type == GGML_TYPE_Q4_K) && op->src[0]->ne[0] % ggml_blck_size(op->type) == 0;
            }
            return true;
        case GGML_OP_MUL_MAT:
            switch (op->src[0]->type) { case GGML_TYPE_F32: case GGML_TYPE_F16: case GGML_TYPE_BF16: case GGML_TYPE_Q4_0: case GGML_TYPE_Q8_0: case GGML_TYPE_Q4_K: return true; default: return false; }
        default: return op->op < GGML_OP_COUNT;
    }
}

static const char * hip_dev_name(ggml_backend_dev_t d) { return ((hip_ctx *) d->context)->name.c_str(); }
static const char * hip_dev_desc(ggml_backend_dev_t d) { return ((hip_ctx *) d->context)->description.c_str(); }
static void hip_dev_memory(ggml_backend_dev_t d, size_t * free, size_t * total) {
    hip_ctx * c = (hip_ctx *) d->context;
    set_device(c);
    if (hipMemGetInfo(free, total) != hipSuccess) { *free = 0; *total = 0; }
}
static enum ggml_backend_dev_type hip_dev_type(ggml_backend_dev_t) { return GGML_BACKEND_DEVICE_TYPE_GPU; }
static ggml_backend_t hip_dev_init(ggml_backend_dev_t d, const char *) {
    hip_ctx * c = (hip_ctx *) d->context;
    ctx_init_lazy(c);
    // a fresh backend handle starts from default flags, the default sampler width and zeroed counters (the device context is shared)
    const int float_acc0 = mmf_env() == 2 ? 1 : 0;   // MI355X_MMF=2: the float-accumulating mat-mul from the start
    if (c->flags != 0 || c->max_columns != 16 || c->float_acc != float_acc0) {
        HIP_CHECK(hipStreamSynchronize(c->stream)); for (auto & kv : c->plans) plan_free(c, kv.second); c->plans.clear(); c->flags = 0; c->max_columns = 16; c->float_acc = float_acc0;
    }
    c->stats = {};
    auto * b = new ggml_backend;
    b->iface = { hip_backend_name, hip_backend_free, hip_backend_sync, hip_alloc_buffer, hip_graph_compute, hip_supports_op, hip_get_tensor_async, hip_event_record, hip_event_wait };
    b->device = d;
    b->context = c;
    return b;
}

static const char * hip_reg_name(ggml_backend_reg_t) { return "ROCm"; }
static size_t hip_reg_dev_count(ggml_backend_reg_t) { return contexts().size(); }
static ggml_backend_dev_t hip_reg_get_dev(ggml_backend_reg_t, size_t i) { return &contexts()[i]->dev_obj; }
static void * hip_reg_proc(ggml_backend_reg_t, const char *) { return NULL; }   // no thread count on a GPU

extern "C" ggml_backend_reg_t ggml_backend_mi355x_reg(void) {
    static ggml_backend_reg reg = { { hip_reg_name, hip_reg_dev_count, hip_reg_get_dev, hip_reg_proc }, NULL };
    static bool init = false;
    if (!init) {
        init = true;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        for (int i = 0; i < n; i++) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, i) != hipSuccess) continue;
            hip_ctx * c = new hip_ctx;
            c->device = i;
            c->name = "ROCm" + std::to_string(i);
            c->description = std::string(prop.name) + " (" + prop.gcnArchName + ")";
            c->dev_obj.iface = { hip_dev_name, hip_dev_desc, hip_dev_memory, hip_dev_type, hip_dev_init };
            c->dev_obj.reg = &reg;
            c->dev_obj.context = c;
            contexts().push_back(c);
        }
    }
    return contexts().empty() ? NULL : &reg;
}

static hip_ctx * ctx_of(ggml_backend_t b) {
    GGML_ASSERT(b && b->iface.get_name == hip_backend_name && "not an MI355X backend");
    return (hip_ctx *) b->context;
}
extern "C" void ggml_backend_mi355x_get_stats(ggml_backend_t b, struct ggml_mi355x_stats * stats) { *stats = ctx_of(b)->stats; }
extern "C" void ggml_backend_mi355x_set_capture(ggml_backend_t b, int enabled) {
    if (b && b->iface.get_name == hip_backend_name) ((hip_ctx *) b->context)->no_capture = !enabled;   // any other backend: nothing to do
}
extern "C" void ggml_backend_mi355x_set_max_columns(ggml_backend_t b, int n) {
    if (b && b->iface.get_name == hip_backend_name) { hip_ctx * c = (hip_ctx *) b->context; n = n < 16 ? 16 : n > SAMPLE_MAX_B ? SAMPLE_MAX_B : n; if (n > c->max_columns) c->max_columns = n; }
}
extern "C" void ggml_backend_mi355x_set_float_accumulate(ggml_backend_t b, int mode) {
    if (!b || b->iface.get_name != hip_backend_name) return;   // any other backend: nothing to do
    hip_ctx * c = (hip_ctx *) b->context;
    mode = mode ? 1 : 0;
    if (mode == c->float_acc) return;
    if (c->stream) { flush_uploads(c); HIP_CHECK(hipStreamSynchronize(c->stream)); }
    for (auto & kv : c->plans) plan_free(c, kv.second);   // the plans hold the other kernel's launches
    c->plans.clear();
    c->float_acc = mode;
}
extern "C" void ggml_backend_mi355x_set_flags(ggml_backend_t b, int flags) {
    hip_ctx * c = ctx_of(b);
    if (c->stream) { flush_uploads(c); HIP_CHECK(hipStreamSynchronize(c->stream)); }
    for (auto & kv : c->plans) plan_free(c, kv.second);
    c->plans.clear();
    c->flags = flags;
}
extern "C" void ggml_backend_mi355x_get_kernel_profile(ggml_backend_t b, struct ggml_mi355x_kernel_profile * out) {
    hip_ctx * c = ctx_of(b);
    out->seconds = c->prof_seconds; out->launches = c->prof_launches; out->bytes = c->prof_bytes;
    for (int v = 0; v < 3; v++) { out->variant_seconds[v] = c->prof_seconds_v[v]; out->variant_launches[v] = c->prof_launches_v[v]; out->variant_bytes[v] = c->prof_bytes_v[v]; }
    out->chain_seconds = c->prof_chain_seconds; out->chain_launches = c->prof_chain_launches; out->chain_bytes = c->prof_chain_bytes; out->chain_phases = c->prof_chain_phases;
}
extern "C" void * ggml_backend_mi355x_get_stream(ggml_backend_t b) { hip_ctx * c = ctx_of(b); ctx_init_lazy(c); return (void *) c->stream; }
// makes the backend's HIP device the calling thread's current one (what a caller that drives another HIP library itself - RCCL's ncclCommInitRank binds the
// communicator to the CURRENT device - needs before it; the backend's own entry points do this internally)
extern "C" void ggml_backend_mi355x_make_current(ggml_backend_t b) { hip_ctx * c = ctx_of(b); ctx_init_lazy(c); set_device(c); }
extern "C" ggml_backend_t ggml_backend_mi355x_init_stream(ggml_backend_t base) {
    if (!base || base->iface.get_name != hip_backend_name) return NULL;   // any other backend: the caller keeps using `base`
    hip_ctx * b0 = (hip_ctx *) base->context;
    hip_ctx * c = nullptr;
    int n_same = 0;
    for (hip_ctx * o : stream_contexts()) if (o->device == b0->device) { n_same++; if (!o->in_use && !c) c = o; }
    if (!c) {
        c = new hip_ctx;
        c->device = b0->device;
        c->name = b0->name + "/s" + std::to_string(n_same + 1);
        c->description = b0->description + ", additional stream";
        c->dev_obj.iface = b0->dev_obj.iface;
        c->dev_obj.reg = b0->dev_obj.reg;
        c->dev_obj.context = c;
        stream_contexts().push_back(c);
    }
    c->in_use = true;
    ggml_backend_t b = c->dev_obj.iface.init_backend(&c->dev_obj, NULL);
    c->flags = b0->flags;             // the debug flags in force on `base` (no fusion / no hipGraph / ...) apply to its sibling stream too
    c->no_capture = b0->no_capture;
    c->max_columns = b0->max_columns;
    c->float_acc = b0->float_acc;     // (a fresh handle holds no plans yet)
    return b;
}
