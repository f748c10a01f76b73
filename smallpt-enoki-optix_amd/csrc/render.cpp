// render.cpp — the render loop behind spt_render* (main.cpp:354-429): the
// working sets, jump tables and queued-render slots of a scene, the enqueue
// of a render as the plan of render_plan.h says, and the first-hit buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <vector>

#include "camera_make.h"
#include "render_plan.h"
#include "scene_state.h"

using namespace spt;

namespace {

// Planes are `stride` elements apart (stride = cap + pad, see queue_stride).
PathQueue carve_queue(char* base, size_t stride, uint32_t planes) {
    PathQueue q;
    float4* f4 = (float4*)base;
    q.q1 = f4;
    q.q2 = f4 + stride;
    q.q0 = planes > 2 ? f4 + 2 * stride : nullptr;
    q.rad = planes > 3 ? (float2*)(f4 + 3 * stride) : nullptr;  // 8 B per path (16 allocated)
    return q;
}

// Plane stride: cap plus a pad (spt_config.plane_pad) so the SoA planes (and
// the two queues) need not sit a power of two apart.
size_t queue_stride(size_t cap, uint32_t pad) { return cap + pad; }

// Device counters of one sub-wavefront (zeroed per chunk; see spt_render).
// The atomically updated counters sit in 128-B lines of their own: a line that
// takes atomics (shade blocks' survivor counts, isect waves' work grabs) slows
// every plain load of the same line from the other waves (config 1 +1.2 %;
// EXPERIMENTS.md, r3_counter_lines).
struct Counters {
    uint32_t qn[2];      // queue counts (isect/shade input)
    alignas(128) uint32_t surv[2];    // survivors appended by shade
    uint64_t cursor[2];  // next work item (double-buffered across refills)
    alignas(128) uint32_t isect_next; // persistent isect work counter (zeroed by each refill)
    uint32_t exhausted;  // RefillArgs::iter_tag of the refill that started the last work item (0: not yet)
    uint32_t pad[2];
    alignas(128) uint32_t xcd_next[8][32];  // the drain / fused kernel's per-XCD work counters (one line each)
    alignas(128) uint32_t surv_shard[kShards][kShardStride];  // a sharded camera cast's survivors per shard
};

// Render-wide device statistics.
struct Stats {
    unsigned long long stats[3];  // casts, continuations, camera rays started
    unsigned long long trav[7];   // SPT_FLAG_TRAVERSAL_STATS: nodes, tris, lane steps, wave steps, max stack,
                                  // wave steps running the triangle block, the visit block
    unsigned long long unwritten; // film slots still holding the sentinel at resolve time
    unsigned long long drained;   // paths finished by drain launches
    unsigned long long drained_casts;  // ray casts traced by drain launches
    // bounce rays the camera casts ended at the BVH root (CameraCastArgs::culled):
    // one counter per shard, each in a line of its own; render_collect sums them
    alignas(128) unsigned long long culled[kShards][kCullStride];
    unsigned long long shadow;    // shadow rays the light-sampling fused kernels traced (kStatShadowWord)
};
constexpr size_t kStatsWords = 13;  // the 64-bit counters before `culled`
static_assert(offsetof(Stats, shadow) == kStatShadowWord * sizeof(unsigned long long),
              "the fused kernel finds the shadow counter from Stats::stats");

// the drain phase starts when the host's (lagging) view of a stream's unstarted
// work falls below this many queue capacities (spt_render_async)
constexpr uint64_t kDrainLookahead = 6;

// One render's own state, so that renders can be queued back to back
// (spt_render_async) while earlier ones are still on the GPU: its device
// counters and their pinned readback, its timing events, and the host-side
// statistics known at enqueue time.  The workspace keeps a ring of them.
constexpr int kRenderSlots = 64;
struct RenderSlot {
    Stats* dev = nullptr;                       // device counters of this render
    Stats* host = nullptr;                      // pinned readback, complete once `done` has fired
    std::vector<hipEvent_t> events;             // [0] = time origin, then start/end pairs of timed launches
    std::vector<std::pair<size_t, int>> timed;  // (start event index, 0 refill 1 isect 2 shade 3 resolve)
    hipEvent_t done = nullptr;                  // recorded after the readback
    spt_render_stats rs{};                      // fields known when the render was queued
    uint64_t regen_base = 0;                    // camera rays of the first launch (for rs.regenerations)
    bool timing = false;
    double wall0 = 0.0;
    uint64_t ticket = 0;
    bool pending = false;                       // queued, not yet collected by spt_render_wait
    bool empty = false;                         // nothing was queued (an empty tile, an empty pixel list)
};

// What a camera entry table (WorkSet::entry) was built for; compared bytewise.
struct EntryKey {
    uint64_t geom_epoch;  // spt_scene_t::geom_epoch: a refit moves the boxes under the same pointers
    const void* nodes;
    uint32_t group_shift;
    spt_camera camera;
    uint32_t width, height, tile_index, tile_count, rows_per_group;
};

// One sub-wavefront: its own double-buffered path queue, hit records and
// counters, driven on its own stream so its launch tails overlap the others'.
struct Sub {
    size_t cap = 0;
    uint32_t pad = 0;                   // plane pad the queues were carved with
    uint32_t planes = 0;                // 16-B planes per path allocated
    char* qa = nullptr;
    char* qb = nullptr;
    char* hits = nullptr;
    Counters* cnt = nullptr;
    hipStream_t stream = nullptr;       // the library's own stream (spt_config.sub_queues)
    // spt_config.drain_sort: sort keys / values (in, out) over cap slots and hipcub scratch
    uint32_t* sort_buf = nullptr;
    size_t sort_cap = 0;
    void* sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    bool own_queue = false;             // created with a full CU mask (spt_config.sub_queues)
    Counters* host_cnt = nullptr;       // pinned, 2 slots (counter snapshots read one batch behind)
    hipEvent_t count_ev[2] = {nullptr, nullptr};
    hipEvent_t join_ev = nullptr;
};

// One render's working memory: path queues, counters and sub-wavefront
// streams, the per-sample film chunk and the running sum.  A scene keeps two
// (kWorkSets), one per caller stream (pick_set), so a render queued on another
// stream can start while the previous one drains; a render waits for the last
// render that used its set (free_ev), so any stream use stays race-free.
constexpr int kWorkSets = 2;
struct WorkSet {
    Sub sub[kMaxStreams];
    hipStream_t home = nullptr;         // the caller stream the set was first used with (bound)
    bool bound = false;
    uint64_t last_ticket = 0;           // the last render that used the set
    size_t film_cap = 0, acc_cap = 0;
    char* film = nullptr;               // per-sample contributions of a chunk (bytes or RGB floats)
    float* acc = nullptr;               // [3][P] running sum across chunks
    // The camera entry table (camera_entry.h): one word per tile pixel, valid
    // for entry_key — the geometry's epoch and nodes, the camera, the image
    // and the tile.  Rebuilt on the set's stream 0 when a render's key differs
    // (ensure_entry), so progressive passes, sample chunks and repeated frames
    // of one view build it once.
    uint32_t* entry = nullptr;
    size_t entry_cap = 0;               // words
    EntryKey entry_key{};
    bool entry_valid = false;
    hipEvent_t fork_ev = nullptr;
    hipEvent_t free_ev = nullptr;       // recorded on the set's stream 0 after the last render that used it
    hipEvent_t call_ev = nullptr;       // the caller stream's work before a render (the render waits for it)
    bool used = false;                  // free_ev has been recorded

    void release() {
        for (Sub& b : sub) {
            hfree(b.qa); hfree(b.qb); hfree(b.hits); hfree(b.cnt); hfree(b.sort_buf);
            if (b.sort_tmp) (void)hipFree(b.sort_tmp);
            if (b.host_cnt) (void)hipHostFree(b.host_cnt);
            for (auto& e : b.count_ev) if (e) (void)hipEventDestroy(e);
            if (b.join_ev) (void)hipEventDestroy(b.join_ev);
            if (b.stream) (void)hipStreamDestroy(b.stream);
        }
        hfree(film); hfree(acc); hfree(entry);
        if (fork_ev) (void)hipEventDestroy(fork_ev);
        if (free_ev) (void)hipEventDestroy(free_ev);
        if (call_ev) (void)hipEventDestroy(call_ev);
        *this = WorkSet();
    }
};

// The PCG32 jump table of one (depth, seed) key: [kMaxDepthCasts] cast jumps,
// then the seeded sample maps of samples [0, n) (read-only while renders run).
// A sample's entry does not depend on the render's spp, so one table serves
// every render and every spt_render_accum pass of its key whose samples end at
// or below n; more samples append a tail (on the render's stream, from the
// table's pinned staging copy) without touching what queued renders read, and
// the table grows geometrically.  A workspace keeps a few, so a caller that
// changes the seed per render reuses them; a table is re-keyed or reallocated
// only after every render that read it has finished — ev[s] is recorded after
// each render of working set s that used the table, and a set's renders run in
// order — and a render on another stream waits for the writes (write_ev; each
// write follows the one before, so the last event covers them all).  No
// device-wide synchronisation.
constexpr int kJumpTables = 4;
struct JumpTable {
    PcgJump* dev = nullptr;
    PcgJump* host = nullptr;            // pinned staging of the last write
    size_t cap = 0;                     // sample entries the buffers hold (after the cast jumps)
    uint32_t n = 0, depth = 0;          // sample entries written
    uint64_t state = 0;
    bool valid = false;
    const PcgJump* casts() const { return dev; }
    const PcgJump* samples() const { return dev + kMaxDepthCasts; }
    uint64_t lru = 0;
    hipEvent_t write_ev = nullptr;
    hipEvent_t ev[kWorkSets] = {};
    bool ev_used[kWorkSets] = {};
    // spt_render_aov reads the table on the caller's stream: aov_ev follows its
    // last launch there (a call on another stream first waits for it, so the
    // one event covers them all)
    hipEvent_t aov_ev = nullptr;
    hipStream_t aov_stream = nullptr;
    bool aov_used = false;
    void release() {
        hfree(dev);
        if (host) (void)hipHostFree(host);
        if (write_ev) (void)hipEventDestroy(write_ev);
        if (aov_ev) (void)hipEventDestroy(aov_ev);
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        *this = JumpTable();
    }
};

}  // namespace

struct spt::Workspace {
    WorkSet sets[kWorkSets];
    // The working set of a render on caller stream `s`: the set bound to that
    // stream, else one never used, else the least recently used (rebound).
    // HIP maps streams onto GPU_MAX_HW_QUEUES (4) hardware queues as they are
    // first used, and a set's sub-wavefront streams were mapped beside the
    // caller stream they first ran with (sub 0 is the caller's own): the same
    // set on another caller stream can put two of the four sub-wavefronts on
    // one queue, which serialises them (config 3 / 4: -17 % / -16 %,
    // profiles/r03_queues/).
    // the set bound to caller stream s, if any (pick_set without binding one)
    const WorkSet* bound_set(hipStream_t s) const {
        for (const WorkSet& w : sets)
            if (w.bound && w.home == s) return &w;
        return nullptr;
    }
    WorkSet& pick_set(hipStream_t s) {
        WorkSet* lru = &sets[0];
        for (WorkSet& w : sets)
            if (w.bound && w.home == s) return w;
        for (WorkSet& w : sets)
            if (!w.bound) {
                w.bound = true;
                w.home = s;
                return w;
            }
        for (WorkSet& w : sets)
            if (w.last_ticket < lru->last_ticket) lru = &w;
        lru->home = s;
        return *lru;
    }
    JumpTable jt[kJumpTables];          // PCG32 jump tables for recent (spp, depth, seed) keys
    uint64_t jt_clock = 0;
    RenderSlot slots[kRenderSlots];     // renders queued by spt_render_async (ticket % kRenderSlots)
    uint64_t next_ticket = 1;
    hipEvent_t epoch = nullptr;         // the first timed render's time origin: isect_begin/end_ms count from it
    // spt_render_accum_list: the list check's verdict on the device and its pinned readback
    uint32_t* list_bad = nullptr;
    uint32_t* list_bad_host = nullptr;
    // spt_debug_entry_table: the set whose camera entry table the last render read (-1: it read none), and its words
    int entry_set = -1;
    uint32_t entry_n = 0;
    // spt_scene_isect_busy_begin/end: every isect [0] and drain [1] launch
    // interval (scene clock) of the renders collected in between, so the union
    // across overlapping queued renders is exact (not one render's span less
    // its overlap)
    bool collect_iv = false;
    // shadow rays of the render collected last (spt_scene_get_shadow_casts)
    uint64_t last_shadow_casts = 0;
    std::vector<std::pair<double, double>> iv_all[2];

    void release() {
        for (WorkSet& w : sets) w.release();
        if (epoch) (void)hipEventDestroy(epoch);
        hfree(list_bad);
        if (list_bad_host) (void)hipHostFree(list_bad_host);
        for (JumpTable& t : jt) t.release();
        for (RenderSlot& r : slots) {
            hfree(r.dev);
            if (r.host) (void)hipHostFree(r.host);
            for (auto e : r.events) (void)hipEventDestroy(e);
            if (r.done) (void)hipEventDestroy(r.done);
        }
        for (auto& v : iv_all) v.clear();
        collect_iv = false;
        const uint64_t t = next_ticket;  // tickets stay unique over the scene's life
        *this = Workspace();
        next_ticket = t;
    }
};

namespace {

// A set's buffers for this render; a buffer that must grow is freed only after
// the last render that used the set has finished with it.
// A sub-wavefront stream of the library's own.  With own_queue, a full CU
// mask: HIP gives a CU-masked stream a hardware queue of its own instead of
// one of the GPU_MAX_HW_QUEUES the process's streams share, so the two working
// sets' sub-wavefronts never serialise behind each other or behind the
// caller's streams on a shared queue.  Falls back to a plain
// non-blocking stream if the runtime refuses the mask.
hipError_t create_sub_stream(hipStream_t* s, bool own_queue) {
    if (own_queue) {
        int dev = 0, cus = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
            std::vector<uint32_t> mask(((uint32_t)cus + 31u) / 32u, 0xffffffffu);
            if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
            if (hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data()) == hipSuccess) return hipSuccess;
            (void)hipGetLastError();
        }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

// spt_debug_root_drain_launches: drains queued through launch_drain_root
std::atomic<uint64_t> g_root_drain_launches{0};
// spt_debug_entry_builds: camera entry tables built (ensure_entry)
std::atomic<uint64_t> g_entry_builds{0};
// spt_debug_fail_workspace_alloc: the allocation that fails once (-1: none)
std::atomic<int32_t> g_fail_ws_alloc{-1};
hipError_t ws_malloc(void** p, size_t bytes) {
    int32_t n = g_fail_ws_alloc.load();
    while (n >= 0 && !g_fail_ws_alloc.compare_exchange_weak(n, n - 1)) {
    }
    if (n == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    return hipMalloc(p, bytes);
}

spt_status ensure_workspace(WorkSet& ws, int nsub, size_t cap, uint32_t pad, uint32_t planes, size_t film_bytes,
                            size_t acc_floats, bool own_queues, bool drain_sort, size_t entry_words) {
    bool quiet = !ws.used;
    const auto quiesce = [&]() -> spt_status {
        if (!quiet) HIP_TRY(hipEventSynchronize(ws.free_ev));
        quiet = true;
        return SPT_OK;
    };
    spt_status st;
    for (int k = 0; k < nsub; k++) {
        Sub& b = ws.sub[k];
        if (cap > b.cap || pad != b.pad || planes > b.planes) {
            if ((st = quiesce())) return st;
            hfree(b.qa); hfree(b.qb); hfree(b.hits);
            b.cap = 0;
            HIP_TRY(ws_malloc((void**)&b.qa, (size_t)16 * planes * queue_stride(cap, pad)));
            HIP_TRY(ws_malloc((void**)&b.qb, (size_t)16 * planes * queue_stride(cap, pad)));
            HIP_TRY(ws_malloc((void**)&b.hits, kHitBytes * cap));
            b.cap = cap;
            b.pad = pad;
            b.planes = planes;
        }
        // spt_config.drain_sort: the forced drain's sort keys / values and hipcub
        // scratch over cap slots, allocated here, where the set is quiesced
        // (not in the middle of an enqueue, behind a host sync)
        if (drain_sort && b.sort_cap < b.cap) {
            if ((st = quiesce())) return st;
            hfree(b.sort_buf);
            if (b.sort_tmp) (void)hipFree(b.sort_tmp);
            b.sort_tmp = nullptr;
            b.sort_cap = 0;
            HIP_TRY(ws_malloc((void**)&b.sort_buf, sizeof(uint32_t) * 4 * b.cap));
            HIP_TRY(launch_drain_sort(DeviceScene{}, PathQueue{}, nullptr, (uint32_t)b.cap, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, &b.sort_tmp_bytes, nullptr));
            HIP_TRY(ws_malloc(&b.sort_tmp, std::max<size_t>(b.sort_tmp_bytes, 16)));
            b.sort_cap = b.cap;
        }
        if (!b.cnt) HIP_TRY(ws_malloc((void**)&b.cnt, sizeof(Counters)));
        if (!b.host_cnt) HIP_TRY(hipHostMalloc((void**)&b.host_cnt, 2 * sizeof(Counters), hipHostMallocDefault));
        for (auto& e : b.count_ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (!b.join_ev) HIP_TRY(hipEventCreateWithFlags(&b.join_ev, hipEventDisableTiming));
        if (b.stream && b.own_queue != own_queues) {  // the stream kind changed (spt_config.sub_queues)
            if ((st = quiesce())) return st;
            HIP_TRY(hipStreamDestroy(b.stream));
            b.stream = nullptr;
        }
        if (!b.stream) {
            HIP_TRY(create_sub_stream(&b.stream, own_queues));
            b.own_queue = own_queues;
        }
    }
    if (film_bytes > ws.film_cap) {
        if ((st = quiesce())) return st;
        hfree(ws.film);
        ws.film_cap = 0;
        HIP_TRY(ws_malloc((void**)&ws.film, film_bytes));
        ws.film_cap = film_bytes;
    }
    if (acc_floats > ws.acc_cap) {
        if ((st = quiesce())) return st;
        hfree(ws.acc);
        ws.acc_cap = 0;
        HIP_TRY(ws_malloc((void**)&ws.acc, sizeof(float) * acc_floats));
        ws.acc_cap = acc_floats;
    }
    if (entry_words > ws.entry_cap) {
        if ((st = quiesce())) return st;
        hfree(ws.entry);
        ws.entry_cap = 0;
        ws.entry_valid = false;
        HIP_TRY(ws_malloc((void**)&ws.entry, sizeof(uint32_t) * entry_words));
        ws.entry_cap = entry_words;
    }
    if (!ws.fork_ev) HIP_TRY(hipEventCreateWithFlags(&ws.fork_ev, hipEventDisableTiming));
    if (!ws.free_ev) HIP_TRY(hipEventCreateWithFlags(&ws.free_ev, hipEventDisableTiming));
    if (!ws.call_ev) HIP_TRY(hipEventCreateWithFlags(&ws.call_ev, hipEventDisableTiming));
    return SPT_OK;
}

// After an allocation that failed: the set's path queues, hit records and film
// chunk are freed (once its last render has finished with them), so a retry
// with fewer paths in flight allocates from scratch.  Streams, counters and
// events stay.
spt_status release_queues(WorkSet& ws) {
    if (ws.used) HIP_TRY(hipEventSynchronize(ws.free_ev));
    for (Sub& b : ws.sub) {
        hfree(b.qa); hfree(b.qb); hfree(b.hits); hfree(b.sort_buf);
        if (b.sort_tmp) (void)hipFree(b.sort_tmp);
        b.sort_tmp = nullptr;
        b.cap = 0;
        b.planes = 0;
        b.sort_cap = 0;
    }
    hfree(ws.film);
    ws.film_cap = 0;
    hfree(ws.entry);
    ws.entry_cap = 0;
    ws.entry_valid = false;
    return SPT_OK;
}

// The PCG32 jump table of a render (JumpTable): from each cast's first draw to
// its bounce draw, 4 + 2 * cast (main.cpp:395,396,413), and to each sample's
// first draw, s * (4 + 2D): seed(initstate, .) then the jump past s * (4 + 2D)
// draws, as one affine map of the stream constant (spt_math.h
// pcg_seeded_jump).  `nsamples`: the table must hold samples [0, nsamples).  A
// hit costs nothing; more samples of a known key write the new tail only; a
// new key rewrites the least recently used table once the renders that read it
// are done, and so does a table outgrown (then at least doubled).
spt_status ensure_jumps(Workspace& w, hipStream_t stream, uint32_t nsamples, uint32_t depth, uint64_t initstate,
                        JumpTable** out) {
    JumpTable* t = nullptr;
    for (JumpTable& x : w.jt)
        if (x.valid && x.depth == depth && x.state == initstate) t = &x;
    const uint64_t per_sample = 4ull + 2ull * depth;
    if (t && nsamples <= t->cap) {
        t->lru = ++w.jt_clock;
        HIP_TRY(hipStreamWaitEvent(stream, t->write_ev, 0));  // written on another stream, perhaps
        if (nsamples > t->n) {
            // the tail: entries nobody reads yet, staged where no copy is in flight
            PcgJump* h = t->host + kMaxDepthCasts;
            for (uint32_t s = t->n; s < nsamples; s++)
                h[s] = pcg_seeded_jump(initstate, pcg_jump_coeffs((uint64_t)s * per_sample));
            HIP_TRY(hipMemcpyAsync(t->dev + kMaxDepthCasts + t->n, h + t->n, sizeof(PcgJump) * (nsamples - t->n),
                                   hipMemcpyHostToDevice, stream));
            HIP_TRY(hipEventRecord(t->write_ev, stream));
            t->n = nsamples;
        }
        *out = t;
        return SPT_OK;
    }
    const bool grow = t != nullptr;  // the key's table, outgrown: its entries stay valid
    if (!t) {
        t = &w.jt[0];
        for (JumpTable& x : w.jt)
            if (!x.valid ? t->valid : x.lru < t->lru) t = &x;
    }
    for (int k = 0; k < kWorkSets; k++)
        if (t->ev_used[k]) HIP_TRY(hipEventSynchronize(t->ev[k]));  // the renders that read it
    if (t->aov_used) HIP_TRY(hipEventSynchronize(t->aov_ev));       // and the spt_render_aov calls
    t->aov_used = false;
    if (t->write_ev) HIP_TRY(hipEventSynchronize(t->write_ev));     // and its last write (staging reuse)
    t->valid = false;
    uint32_t have = grow ? t->n : 0;
    if (nsamples > t->cap) {
        const size_t cap = std::max<size_t>(std::max<size_t>(nsamples, 2 * t->cap), 64);
        PcgJump* dev = nullptr;
        PcgJump* host = nullptr;
        HIP_TRY(hipMalloc((void**)&dev, sizeof(PcgJump) * (cap + kMaxDepthCasts)));
        if (hipHostMalloc((void**)&host, sizeof(PcgJump) * (cap + kMaxDepthCasts), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            hfree(dev);
            return fail(SPT_ERR_OOM, "spt_render: no pinned memory for the jump table");
        }
        if (have) memcpy(host + kMaxDepthCasts, t->host + kMaxDepthCasts, sizeof(PcgJump) * have);
        hfree(t->dev);
        if (t->host) (void)hipHostFree(t->host);
        t->dev = dev;
        t->host = host;
        t->cap = cap;
    }
    if (!t->write_ev) HIP_TRY(hipEventCreateWithFlags(&t->write_ev, hipEventDisableTiming));
    for (auto& e : t->ev)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (uint32_t j = 0; j < kMaxDepthCasts; j++) t->host[j] = pcg_jump_coeffs(4ull + 2ull * j);
    PcgJump* h = t->host + kMaxDepthCasts;
    for (uint32_t s = have; s < nsamples; s++) h[s] = pcg_seeded_jump(initstate, pcg_jump_coeffs((uint64_t)s * per_sample));
    HIP_TRY(hipMemcpyAsync(t->dev, t->host, sizeof(PcgJump) * ((size_t)kMaxDepthCasts + nsamples), hipMemcpyHostToDevice,
                           stream));
    HIP_TRY(hipEventRecord(t->write_ev, stream));
    for (bool& u : t->ev_used) u = false;
    t->n = nsamples;
    t->depth = depth;
    t->state = initstate;
    t->valid = true;
    t->lru = ++w.jt_clock;
    *out = t;
    return SPT_OK;
}

spt_status get_event(RenderSlot& r, size_t idx, hipEvent_t* out) {
    while (r.events.size() <= idx) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        r.events.push_back(e);
    }
    *out = r.events[idx];
    return SPT_OK;
}

// The slot of the next render; SPT_ERR_LIMIT when the render kRenderSlots
// tickets earlier was never collected.
spt_status render_slot(Workspace& ws, RenderSlot** out) {
    RenderSlot& r = ws.slots[ws.next_ticket % kRenderSlots];
    if (r.pending)
        return fail(SPT_ERR_LIMIT, "spt_render_async: %d renders queued without spt_render_wait", kRenderSlots);
    if (!r.dev) HIP_TRY(hipMalloc((void**)&r.dev, sizeof(Stats)));
    if (!r.host) HIP_TRY(hipHostMalloc((void**)&r.host, sizeof(Stats), hipHostMallocDefault));
    if (!r.done) HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
    r.timed.clear();
    r.rs = spt_render_stats{};
    r.timing = false;
    r.empty = false;
    *out = &r;
    return SPT_OK;
}

// Total length of a set of intervals (their union), sorted by start.
template <typename T>
double interval_union(const std::vector<std::pair<T, T>>& iv) {
    double busy = 0.0, lo = 0.0, hi = -1.0;
    for (auto& x : iv) {
        if (x.first > hi) {
            if (hi > lo) busy += hi - lo;
            lo = x.first;
            hi = x.second;
        } else {
            hi = std::max<double>(hi, x.second);
        }
    }
    if (hi > lo) busy += hi - lo;
    return busy;
}

// Waits for a queued render and fills its statistics (device counters, the
// union of its isect launch intervals, host wall time since it was queued).
spt_status render_collect(RenderSlot& r, Workspace& ws, spt_render_stats* out) {
    const hipEvent_t epoch = ws.epoch;
    spt_render_stats rs = r.rs;
    r.pending = false;
    if (rs.tile_rows && !r.empty) {  // an empty tile (or pixel list) queued nothing
        HIP_TRY(hipEventSynchronize(r.done));
        const unsigned long long* hstats = reinterpret_cast<const unsigned long long*>(r.host);
        static_assert(offsetof(Stats, culled) >= kStatsWords * sizeof(unsigned long long) &&
                          offsetof(Stats, drained_casts) == (kStatsWords - 1) * sizeof(unsigned long long),
                      "Stats is the 13 counters read back here, then the culled shards");
        // A culled bounce ray is a cast that was traced and ended in a miss, in
        // the camera cast's launch: a cast and the continuation that led to it,
        // as if the drain had traced it, but not drained.  (lockstep_casts stays
        // the first casts: ray_casts - drained_casts == lockstep_casts + culled_paths
        // where the camera cast ran.)
        unsigned long long culled = 0;
        for (uint32_t j = 0; j < kShards; j++) culled += r.host->culled[j][0];
        rs.ray_casts = hstats[0] + culled;
        rs.continuations = hstats[1] + culled;
        rs.culled_paths = (uint32_t)std::min<unsigned long long>(culled, 0xffffffffull);
        rs.regenerations = hstats[2] > r.regen_base ? hstats[2] - r.regen_base : 0;
        rs.isect_nodes = hstats[3];
        rs.isect_tris = hstats[4];
        rs.isect_lane_steps = hstats[5];
        rs.isect_wave_steps = hstats[6];
        rs.isect_max_stack = hstats[7];
        rs.paths_started = hstats[2];
        rs.paths_terminated = hstats[0] - hstats[1];  // every cast either continues or ends its path
        rs.paths = rs.paths_terminated;
        rs.film_slots_unwritten = hstats[10];
        rs.isect_tri_wave_steps = hstats[8];
        rs.isect_node_wave_steps = hstats[9];
        rs.drained_paths = hstats[11];
        rs.drained_casts = hstats[12];
        ws.last_shadow_casts = r.host->shadow;
        if (r.timing) {
            uint64_t nis = 0;
            // launch intervals from the origin: [0] isect (the fused kernel in
            // the fused pipeline), [1] the wavefront's drain
            std::vector<std::pair<float, float>> iv[2];
            for (auto& tk : r.timed) {
                float ms = 0.0f;
                HIP_TRY(hipEventElapsedTime(&ms, r.events[tk.first], r.events[tk.first + 1]));
                if (tk.second == 0) rs.camera_ms += ms;
                else if (tk.second == 1 || tk.second == 4) {
                    float t0 = 0.0f;
                    HIP_TRY(hipEventElapsedTime(&t0, r.events[0], r.events[tk.first]));
                    if (tk.second == 1) {
                        rs.isect_ms += ms;
                        nis++;
                    } else {
                        rs.drain_ms += ms;
                    }
                    iv[tk.second == 4].push_back({t0, t0 + ms});
                } else if (tk.second == 2) rs.shade_ms += ms;
                else rs.resolve_ms += ms;
            }
            rs.isect_launches = nis;
            // launches on the K streams overlap: busy time = union of their intervals
            for (auto& v : iv) std::sort(v.begin(), v.end());
            if (!iv[0].empty() && epoch) {  // the span on the scene's clock, for unions across queued renders
                float t_origin = 0.0f;
                HIP_TRY(hipEventElapsedTime(&t_origin, epoch, r.events[0]));
                float last = iv[0][0].second;
                for (auto& x : iv[0]) last = std::max(last, x.second);
                rs.isect_begin_ms = (double)t_origin + iv[0][0].first;
                rs.isect_end_ms = (double)t_origin + last;
                if (ws.collect_iv)
                    for (int k = 0; k < 2; k++)
                        for (auto& x : iv[k])
                            ws.iv_all[k].push_back({(double)t_origin + x.first, (double)t_origin + x.second});
            }
            rs.isect_busy_ms = interval_union(iv[0]);
            rs.drain_busy_ms = interval_union(iv[1]);
        }
    }
    rs.total_ms = now_ms() - r.wall0;
    if (out) *out = rs;
    return SPT_OK;
}

}  // namespace

namespace spt {

Workspace* workspace_new() { return new Workspace(); }
void workspace_release(Workspace& ws) { ws.release(); }
void workspace_delete(Workspace* ws) {
    ws->release();
    delete ws;
}

// (see PublicUse) caller holds sc->mu
spt_status quiesce_scene(spt_scene_t* sc) {
    for (WorkSet& w : sc->ws.sets)
        if (w.used && w.free_ev) HIP_TRY(hipEventSynchronize(w.free_ev));
    for (auto& u : sc->pub) HIP_TRY(hipEventSynchronize(u.ev));
    return SPT_OK;
}

}  // namespace spt

namespace {

// ---------------------------------------------------------------- the enqueue

// Byte ranges [a, a + n) and [b, b + n) overlap (either may be null: no range).
bool ranges_overlap(const void* a, const void* b, uint64_t n) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x < n : x - y < n;
}

// Byte ranges [a, a + na) and [b, b + nb) overlap (either may be null or empty: no range).
bool ranges_overlap2(const void* a, uint64_t na, const void* b, uint64_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x < na : x - y < nb;
}

// The argument checks of spt_render_async (accum_call false),
// spt_render_accum_async and spt_render_accum_list (list_call); *rows_out: the
// tile's rows.
spt_status check_render_args(spt_scene sc, const spt_render_params* pp, const float* film_dev, const spt_accum* accum,
                             bool accum_call, const uint64_t* ticket_out, uint32_t* rows_out,
                             const spt_pixel_list* list = nullptr, bool list_call = false) {
    if (list_call) {
        if (!list) return fail(SPT_ERR_INVALID, "spt_render_accum_list: NULL list");
        if (list->reserved != 0) return fail(SPT_ERR_INVALID, "spt_render_accum_list: reserved must be 0");
        if (list->n && !list->pixels) return fail(SPT_ERR_INVALID, "spt_render_accum_list: NULL pixels");
    }
    if (!sc || !pp || !ticket_out) return fail(SPT_ERR_INVALID, "spt_render: NULL argument");
    if (accum_call) {
        if (!accum || !accum->sum) return fail(SPT_ERR_INVALID, "spt_render_accum: NULL accumulator / sum");
        if (accum->reserved != 0) return fail(SPT_ERR_INVALID, "spt_render_accum: reserved must be 0");
        if (accum->variance && !accum->sum_sq)
            return fail(SPT_ERR_INVALID, "spt_render_accum: variance needs sum_sq");
    }
    const spt_render_params& p = *pp;
    if (p.width == 0 || p.height == 0 || p.spp == 0 || p.max_depth == 0)
        return fail(SPT_ERR_INVALID, "spt_render: width/height/spp/max_depth must be > 0");
    if (p.max_depth > kMaxDepthCasts) return fail(SPT_ERR_LIMIT, "spt_render: max_depth %u > %u", p.max_depth, kMaxDepthCasts);
    if (p.spp >= (1u << 24)) return fail(SPT_ERR_LIMIT, "spt_render: spp must be < 2^24");
    if ((uint64_t)p.width * p.height >= (1ull << 31)) return fail(SPT_ERR_LIMIT, "spt_render: image too large");
    if (p.tile_count == 0 || p.rows_per_group == 0 || p.tile_index >= p.tile_count)
        return fail(SPT_ERR_INVALID, "spt_render: bad tile (%u of %u, %u rows/group)", p.tile_index, p.tile_count,
                    p.rows_per_group);
    if (p.rng_order > 1) return fail(SPT_ERR_INVALID, "spt_render: rng_order must be 0 or 1");
    const uint32_t rows = spt_tile_rows(p.height, p.tile_index, p.tile_count, p.rows_per_group, nullptr, 0);
    const uint64_t P = (uint64_t)rows * p.width;
    if (P != 0 && !film_dev && !accum) return fail(SPT_ERR_INVALID, "spt_render: NULL film");
    if (accum) {
        // n = sample_base + spp stays exact in f32
        if ((uint64_t)accum->sample_base + p.spp >= (1ull << 24))
            return fail(SPT_ERR_LIMIT, "spt_render_accum: sample_base + spp must be < 2^24");
        const void* planes[4] = {accum->sum, accum->sum_sq, accum->film, accum->variance};
        for (int i = 0; i < 4; i++)
            for (int j = i + 1; j < 4; j++)
                if (planes[i] && (planes[i] == planes[j] || ranges_overlap(planes[i], planes[j], 12ull * P)))
                    return fail(SPT_ERR_INVALID, "spt_render_accum: sum, sum_sq, film and variance must not overlap");
        if (list_call) {
            if (list->n > P)
                return fail(SPT_ERR_INVALID, "spt_render_accum_list: %u listed pixels, the tile has %llu", list->n,
                            (unsigned long long)P);
            if (((uintptr_t)list->pixels | (uintptr_t)list->count) & 3u)
                return fail(SPT_ERR_INVALID, "spt_render_accum_list: pixels and count must be 4-byte aligned");
            const uint64_t nl = 4ull * list->n, nc = 4ull * P;
            bool bad = ranges_overlap2(list->pixels, nl, list->count, nc);
            for (int i = 0; i < 4; i++)
                bad = bad || ranges_overlap2(planes[i], 12ull * P, list->pixels, nl) ||
                      ranges_overlap2(planes[i], 12ull * P, list->count, nc);
            if (bad)
                return fail(SPT_ERR_INVALID, "spt_render_accum_list: pixels and count must not overlap each other or "
                            "sum, sum_sq, film, variance");
        }
    }
    *rows_out = rows;
    return SPT_OK;
}

// RenderPlanIn::free_bytes: the device's free memory
bool device_free_bytes(void*, uint64_t* out) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    *out = fr;
    return true;
}

// What plan_render reads of this render (render_plan.h).
RenderPlanIn plan_inputs(const spt_scene_t* sc, const spt_render_params& p, uint64_t P, uint64_t A,
                         hipStream_t caller) {
    RenderPlanIn in;
    in.A = A;
    in.P = P; in.spp = p.spp; in.flags = p.flags; in.wavefront_paths = p.wavefront_paths;
    in.cfg = &sc->cfg;
    // What a path carries (spt_internal.h PathMode): the reference's case
    // (every albedo 1, no emitters) needs only the ray and an escaped flag.
    // (a sky image needs radiance in the film slots: an escaped flag cannot carry it)
    const bool unit = sc->albedo_unit && sc->ntex == 0 && sc->nsph == 0 && sc->nkind == 0 && !sc->envmap;
    // (a scene that samples its sky takes the emitter-mode instances, the only ones
    // with the light-sampling lane loop, with or without an emission table)
    in.mode = sc->emission || sc->sky ? kModeEmit : (unit ? kModeUnit : kModeAlbedo);
    in.planes = mode_planes(in.mode);
    in.film_unit = mode_film_bytes(in.mode);
    in.device_bytes = sc->stats.device_bytes;
    in.nsph = sc->nsph;
    in.wide_nodes = sc->nodes8 != nullptr;
    in.node6 = sc->node6 != 0;
    in.pinhole = p.camera.lens_radius == 0.0f;
    in.nee = sc->lights != nullptr || sc->sky != nullptr;
    in.null_caller = caller == nullptr || caller == hipStreamLegacy || caller == hipStreamPerThread;
    if (const WorkSet* hs = sc->ws.bound_set(caller)) {
        for (int k = 0; k < kMaxStreams; k++) {
            const Sub& b = hs->sub[k];
            in.held_sub[k] = 2ull * 16 * b.planes * queue_stride(b.cap, b.pad) + kHitBytes * b.cap;
        }
        in.held_film = hs->film_cap;
        in.held_entry = sizeof(uint32_t) * hs->entry_cap;
    }
    in.free_bytes = device_free_bytes;
    return in;
}

// From the first launch on, work is queued on the set's streams.  Any early
// return (a failed launch, a queue that did not drain) still joins the
// sub-wavefront streams into `stream` and records free_ev, so the next
// render that picks this set waits for whatever this one left running.
struct EnqueueGuard {
    WorkSet& ws;
    hipStream_t stream, caller;
    JumpTable& jt;
    int set = 0;
    int K = 1;
    bool armed = true;
    ~EnqueueGuard() {
        if (!armed) return;
        for (int k = 1; k < K; k++) {
            (void)hipEventRecord(ws.sub[k].join_ev, ws.sub[k].stream);
            (void)hipStreamWaitEvent(stream, ws.sub[k].join_ev, 0);
        }
        (void)hipEventRecord(ws.free_ev, stream);
        (void)hipEventRecord(jt.ev[set], stream);
        (void)hipStreamWaitEvent(caller, ws.free_ev, 0);
        jt.ev_used[set] = true;
        ws.used = true;
    }
};

// One sub-wavefront's run of a sample chunk: its kernel arguments (queues and
// counters differ between sub-wavefronts) and the host's view of its progress.
struct SubRun {
    IsectQueueArgs ia;
    ShadeArgs sa;
    RefillArgs ra;
    FusedArgs da;          // the drain launches (launch_drain)
    PathQueue q[2];
    uint32_t drain_T;      // the drain takes a queue shorter than this
    uint32_t known;        // paths in the queue, as last read back
    int cur;               // the queue the next isect reads
    int pending, pend_cur; // the counter snapshot in flight (-1: none) and the queue it describes
    uint64_t pend_it;
    uint64_t limit;        // the iteration the queue is empty by (UINT64_MAX: not known yet)
    bool live;
    uint64_t started, sub_begin, sub_end;  // work items known started; the share
    bool lock0;            // the first cast runs in lockstep
    bool root_words;       // the camera cast left its survivors' root-visit words in the hit records'
                           // buffer for the forced drain that comes next (RenderPlan::root_handoff)
};

// What the pieces of one enqueue share.
struct RenderJob {
    spt_scene_t* sc;
    const spt_render_params& p;
    const RenderPlan& pl;
    WorkSet& ws;
    RenderSlot& slot;
    float* film_dev;
    const spt_accum* accum;
    uint64_t P;
    // the pixels that take samples: P, or the n of spt_render_accum_list's list
    // (work items count A per sample; film slots stay P per sample)
    uint64_t A;
    const spt_pixel_list* list;
    uint32_t s_begin, s_end;  // the samples [sample_base, sample_base + spp)
    const PcgJump *jumps, *cjumps;
    Camera cam;
    hipStream_t stream;       // the set's stream 0
    // HIP events around the isect launches (the roofline kernel); every other
    // launch only with SPT_FLAG_TIMING_ALL (each event pair costs host time).
    bool timing, timing_all;
    size_t ev = 1;            // events[0] is the origin
    uint64_t drain_launches = 0;
    const uint32_t* entry = nullptr;  // the camera entry table of this view (ensure_entry; null: none)

    const spt_config& cfg() const { return sc->cfg; }
    float* sfilm() const { return (float*)ws.film; }
    uint8_t* sflag() const { return (uint8_t*)ws.film; }

    // kind: 0 refill 1 isect 2 shade 3 resolve 4 drain
    template <typename Launch>
    spt_status mark(int kind, hipStream_t sk, Launch&& launch) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        spt_status s2;
        const bool tm = (kind == 1 || kind == 4) ? timing : timing_all;  // isect and drain: the tracing kernels
        if (tm) {
            if ((s2 = get_event(slot, ev, &e0)) || (s2 = get_event(slot, ev + 1, &e1))) return s2;
            HIP_TRY(hipEventRecord(e0, sk));
        }
        HIP_TRY(launch());
        if (tm) {
            HIP_TRY(hipEventRecord(e1, sk));
            slot.timed.push_back({ev, kind});
            ev += 2;
        }
        return SPT_OK;
    }

    // film slots follow the work order (film_slot)
    hipError_t resolve(uint32_t s0, uint32_t ns) const {
        const uint32_t film_order = pl.pixel_major;
        if (accum) {
            ResolveAccumArgs ra{};
            ra.sum = accum->sum; ra.sum_sq = accum->sum_sq; ra.film = accum->film; ra.variance = accum->variance;
            ra.P = (uint32_t)P; ra.nsamples = ns;
            ra.from_zero = s0 == 0;
            ra.last = s0 + ns >= s_end;
            ra.n_total = s_end;
            ra.order = film_order;
            ra.env_r = p.env[0]; ra.env_g = p.env[1]; ra.env_b = p.env[2];
            ra.unwritten = &slot.dev->unwritten;
            if (list) {
                const ResolveListArgs la{ra, list->pixels, list->n, list->count};
                return pl.mode == kModeUnit ? launch_resolve_flags_accum_list(sflag(), la, stream)
                                            : launch_resolve_accum_list(sfilm(), la, stream);
            }
            return pl.mode == kModeUnit ? launch_resolve_flags_accum(sflag(), ra, stream)
                                        : launch_resolve_accum(sfilm(), ra, stream);
        }
        return pl.mode == kModeUnit
                   ? launch_resolve_flags(sflag(), ws.acc, film_dev, (uint32_t)P, ns, s0 == 0, s0 + ns >= p.spp, p.spp,
                                          p.env[0], p.env[1], p.env[2], film_order, &slot.dev->unwritten, stream)
                   : launch_resolve(sfilm(), ws.acc, film_dev, (uint32_t)P, ns, s0 == 0, s0 + ns >= p.spp, p.spp,
                                    film_order, &slot.dev->unwritten, stream);
    }
    // every slot of a chunk starts as the sentinel (kFlagSentinel / kFilmSentinel
    // bytes), so the resolve counts slots no path wrote (spt_render_stats)
    hipError_t clear_film(uint32_t ns) const {
        return hipMemsetAsync(ws.film, 0xff, (size_t)ns * mode_film_bytes(pl.mode) * P, stream);
    }
    // drain_casts after the exhausting refill (limit - max_depth) the drain
    // runs whatever the queue holds, and the stream ends: no work is left to
    // start, so nothing can enter its queue again (both `force` and the camera
    // cast's `sharded` in run_iteration depend on this)
    bool forced_at(const SubRun& r, uint64_t iter) const {
        return pl.drain_on && cfg().drain_casts && r.limit != UINT64_MAX &&
               iter + p.max_depth >= r.limit + cfg().drain_casts;
    }
};

// The fields RefillArgs, ShadeArgs and FusedArgs have in common: the tile,
// the image and the RNG ...
template <typename Args>
void fill_tile_args(Args& a, const RenderJob& j) {
    a.sample_jump = j.jumps;
    a.initstate = j.p.rng_initstate;
    a.P = (uint32_t)j.P; a.W = j.p.width; a.rng_order = j.p.rng_order;
    a.tile_index = j.p.tile_index; a.tile_count = j.p.tile_count; a.rows_per_group = j.p.rows_per_group;
}
// ... and those of the two that shade: the scene, the film chunk, the cast
// jumps, the depth and roulette limits, the environment
template <typename Args>
void fill_shade_args(Args& a, const RenderJob& j) {
    fill_tile_args(a, j);
    a.sc = j.sc->dev();
    a.sfilm = j.sfilm();
    a.sflag = j.sflag();
    a.cast_jump = j.cjumps;
    a.max_depth = j.p.max_depth; a.rr_start = j.p.rr_start_depth;
    a.env_r = j.p.env[0]; a.env_g = j.p.env[1]; a.env_b = j.p.env[2];
}

// The lane loop's arguments (render_fused_kernel): the fused pipeline's
// launches, or with `drain` the drain launches of a sub-wavefront.
FusedArgs lane_loop_args(const RenderJob& j, const Sub& b, bool drain) {
    const spt_config& cfg = j.cfg();
    FusedArgs F{};
    fill_shade_args(F, j);
    F.cam = j.cam;
    if (j.list && !drain) {
        F.list = j.list->pixels;
        F.list_n = j.list->n;
    }
    F.stats = j.slot.dev->stats;
    F.next = &b.cnt->isect_next;  // (drain: zeroed by the refill before; an isect that skips leaves it)
    F.xcd_next = j.pl.lane_xcd ? &b.cnt->xcd_next[0][0] : nullptr;  // (drain: zeroed by the refill before)
    // a small static share: the fused lanes' path lengths vary far more
    // than one cast's, so most work is taken dynamically (1/8 tile of
    // config 1: 32/256 3006, 0: 2938, 64: 2912, 160: 2558 Mpaths/s)
    F.static_share_q8 = cfg.fused_static_share_q8;
    F.chunk = cfg.isect_chunk;
    if (drain) {
        F.drained = &j.slot.dev->drained;
        F.drained_casts = &j.slot.dev->drained_casts;
        F.refill_idle = j.pl.drain_idle;
        F.grid_q8 = cfg.drain_grid_q8 ? cfg.drain_grid_q8 : 256u / (uint32_t)j.pl.K;
        F.nt = j.pl.queue_nt;
    } else {
        F.refill_idle = cfg.fused_refill_idle;
        F.grid_q8 = cfg.fused_grid_q8;
    }
    return F;
}

// Sub-wavefront k's arguments for the whole render (what changes per chunk
// and per iteration is set there).
void init_sub_run(SubRun& r, const RenderJob& j, const Sub& b) {
    const spt_config& cfg = j.cfg();
    const RenderPlan& pl = j.pl;
    r = SubRun{};
    r.q[0] = carve_queue(b.qa, queue_stride(b.cap, b.pad), mode_planes(pl.mode));
    r.q[1] = carve_queue(b.qb, queue_stride(b.cap, b.pad), mode_planes(pl.mode));
    IsectQueueArgs& I = r.ia;
    I.sc = j.sc->dev();
    I.hits = (float4*)b.hits;
    I.nt = pl.queue_nt && !pl.trav_stats;
    I.max_depth = j.p.max_depth;
    I.trav_stats = pl.trav_stats ? j.slot.dev->trav : nullptr;
    I.next = &b.cnt->isect_next;
    // 24 idle lanes / a 1/2 static share: +1.5 % over 16 / 5/8 at the
    // 32M wavefront (tools/envsweep.sh, tools/envsweep_r01_v11.txt)
    I.refill_idle = cfg.isect_refill_idle;
    I.static_share_q8 = cfg.isect_static_share_q8;
    I.xcd_remap = cfg.xcd_remap & 1u;
    I.chunk = cfg.isect_chunk;
    // each stream's persistent grid covers 1/K of the chip (measured best)
    I.grid_q8 = cfg.isect_grid_q8 ? cfg.isect_grid_q8 : 256u / (uint32_t)pl.K;
    ShadeArgs& S = r.sa;
    fill_shade_args(S, j);
    S.hits = (const float4*)b.hits;
    S.xcd_remap = (cfg.xcd_remap >> 1) & 1u;
    S.work_order = pl.pixel_major;
    S.nt = pl.queue_nt;
    RefillArgs& R = r.ra;
    fill_tile_args(R, j);
    R.cam = j.cam;
    if (j.list) {
        R.list = j.list->pixels;
        R.list_n = j.list->n;
    }
    R.stats = j.slot.dev->stats;
    R.capacity = (uint32_t)b.cap;
    R.pixel_block = cfg.pixel_block;
    R.work_order = pl.pixel_major;
    R.nt = pl.queue_nt;
    R.mode = pl.mode;
    R.isect_next = &b.cnt->isect_next;
    R.exhausted = &b.cnt->exhausted;
    R.xcd_next = pl.lane_xcd ? &b.cnt->xcd_next[0][0] : nullptr;
    if (pl.drain_on) {
        // a queue shorter than drain_q8/256 of this stream's isect lanes
        r.drain_T = (uint32_t)std::min<uint64_t>(0xffffffffull, (uint64_t)isect_queue_lanes(I) * cfg.drain_q8 / 256u);
        r.da = lane_loop_args(j, b, true);
    }
}

// The fused pipeline: one launch of the persistent kernel and a resolve per
// sample chunk.  *lanes: the lanes of the launches (the paths in flight).
spt_status enqueue_fused(RenderJob& j, uint64_t* iters, uint32_t* lanes) {
    FusedArgs F = lane_loop_args(j, j.ws.sub[0], false);
    const int mode = j.pl.mode;
    spt_status st;
    for (uint32_t s0 = j.s_begin; s0 < j.s_end; s0 += j.pl.chunk) {
        const uint32_t ns = std::min(j.pl.chunk, j.s_end - s0);
        F.work0 = (uint64_t)s0 * j.A;
        F.count = (uint32_t)((uint64_t)ns * j.A);  // <= 4 GiB / 12 B per chunk
        F.sample0 = s0;
        F.pm_ns = j.pl.pixel_major ? ns : 0;
        HIP_TRY(j.clear_film(ns));
        HIP_TRY(hipMemsetAsync(F.next, 0, sizeof(uint32_t), j.stream));
        if (F.xcd_next) HIP_TRY(hipMemsetAsync(F.xcd_next, 0, sizeof(uint32_t) * 8 * 32, j.stream));
        if ((st = j.mark(1, j.stream, [&] { return launch_fused(F, mode, j.stream, lanes); }))) return st;
        if ((st = j.mark(3, j.stream, [&] { return j.resolve(s0, ns); }))) return st;
        (*iters)++;
    }
    return SPT_OK;
}

// A chunk's first refill of sub-wavefront k: its share of the chunk's work
// items [w0, w0 + L), the counters zeroed, the first paths started.
spt_status first_refill(RenderJob& j, SubRun& r, int k, uint32_t s0, uint32_t ns) {
    const RenderPlan& pl = j.pl;
    Sub& b = j.ws.sub[k];
    const hipStream_t sk = b.stream;
    const int K = pl.K;
    const uint64_t w0 = (uint64_t)s0 * j.A, L = (uint64_t)ns * j.A;
    // contiguous share of the chunk's work items (sample-major); pixel-major
    // work splits the chunk's samples instead, so that every stream
    // covers the whole tile (a band of rows per stream would leave the
    // streams unevenly loaded) and starts its samples of a pixel together
    uint64_t wb = w0 + L * k / K, we = w0 + L * (k + 1) / K;
    r.ra.chunk_s0 = s0; r.ra.chunk_ns = ns;
    if (r.ra.work_order && ns >= (uint32_t)K) {
        const uint32_t sk0 = s0 + ns * k / K, sk1 = s0 + ns * (k + 1) / K;
        wb = (uint64_t)sk0 * j.A; we = (uint64_t)sk1 * j.A;
        r.ra.chunk_s0 = sk0; r.ra.chunk_ns = sk1 - sk0;
    }
    HIP_TRY(hipMemsetAsync(b.cnt, 0, sizeof(Counters), sk));
    r.ra.work_end = we;
    r.sa.sample0 = s0; r.sa.chunk_ns = ns;
    r.da.sample0 = s0; r.da.pm_ns = pl.pixel_major ? ns : 0;  // the shade's film layout
    r.da.seg_count = nullptr;  // (set by a sharded camera cast of this chunk)
    r.da.xcd_next = pl.lane_xcd ? &b.cnt->xcd_next[0][0] : nullptr;
    // the first refill starts at the sub-wavefront's first work item
    r.ra.q = r.q[0]; r.ra.surv = &b.cnt->surv[0]; r.ra.cursor_in = nullptr; r.ra.cursor_init = wb;
    r.ra.cursor_out = &b.cnt->cursor[0]; r.ra.qn_out = &b.cnt->qn[0];
    r.ra.surv_clear = nullptr;
    r.ra.casts_in = nullptr;
    r.ra.iter_tag = 1;
    const uint32_t first = (uint32_t)std::min<uint64_t>(b.cap, we - wb);
    r.sub_begin = wb;
    r.sub_end = we;
    r.started = wb + first;
    // spt_config.lockstep_first: the first cast of a fitting job — every
    // path started by the first refill, the count known exactly and long
    // enough that the isect and shade run (not the drain) — in the
    // one-lane-per-ray kernel (launch_isect_lockstep)
    r.lock0 = j.cfg().lockstep_first && pl.fit && pl.drain_on && !pl.trav_stats && first >= r.drain_T;
    r.root_words = false;
    // (the camera cast makes these paths itself: the refill only keeps the books)
    r.ra.book_only = r.lock0 && pl.cam_cast ? 1u : 0u;
    spt_status st;
    if ((st = j.mark(0, sk, [&] { return launch_refill(r.ra, r.ra.book_only ? 1u : first, sk); }))) return st;
    r.ra.book_only = 0;
    r.known = (uint32_t)std::min<uint64_t>(b.cap, r.started - r.sub_begin);
    r.cur = 0;
    r.pending = -1;
    r.pend_cur = 0;
    r.pend_it = 0;
    // everything fit in the first refill: exactly max_depth iterations
    r.limit = r.started >= r.sub_end ? j.p.max_depth : UINT64_MAX;
    r.live = r.known > 0;
    return SPT_OK;
}

// Iteration `it` of sub-wavefront k: isect -> shade -> (drain) -> refill, or
// the forced drain that ends the stream.
spt_status run_iteration(RenderJob& j, SubRun& r, int k, uint64_t it) {
    const RenderPlan& pl = j.pl;
    const int mode = pl.mode;
    if (it >= r.limit) {  // drained by construction
        r.live = false;
        return SPT_OK;
    }
    Sub& b = j.ws.sub[k];
    const hipStream_t sk = b.stream;
    spt_status st;
    const int c = r.cur, nx = 1 - c;
    r.ia.q = r.q[c];
    r.ia.count = &b.cnt->qn[c];
    // The drain phase: once the stream's last work items are (about
    // to be) started — the host's view lags one or two batches, in
    // which the cursor moves < kDrainLookahead capacities — a drain
    // launch follows the shade.  Whichever sees the queue short
    // (< drain_T) runs: the isect and shade skip and the drain
    // finishes every queued path, or the drain skips.  Later
    // iterations find the queue empty (no-op launches).
    const bool dph = pl.drain_on &&
                     (r.limit != UINT64_MAX || r.sub_end - r.started < kDrainLookahead * (uint64_t)b.cap);
    const bool force = j.forced_at(r, it);
    r.ia.drain_below = force ? 0xffffffffu : dph ? r.drain_T : 0u;
    r.sa.drain_below = r.ia.drain_below;
    if (force) {
        r.da.q = r.q[c];
        r.da.qcount = &b.cnt->qn[c];
        r.da.drain_below = 0xffffffffu;
        r.da.perm = nullptr;
        if (pl.drain_sort) {  // the drain's order: by direction octant, then origin (kernels.hip)
            const size_t cap = b.cap;  // (buffers: ensure_workspace)
            uint32_t* kb = b.sort_buf;
            HIP_TRY(launch_drain_sort(j.sc->dev(), r.q[c], &b.cnt->qn[c], (uint32_t)b.cap, kb, kb + cap, kb + 2 * cap,
                                      kb + 3 * cap, b.sort_tmp, &b.sort_tmp_bytes, sk));
            r.da.perm = kb + 3 * cap;
        }
        // (the drain counts the queued paths' first casts itself: the stream
        // ends here, and a bookkeeping refill behind it would wait for CU
        // slots behind the other working set's persistent drain, 0.4 ms on
        // the 1/8 tile, profiles/r06_exp/tile8_trace/)
        r.da.count_queue = 1;
        const bool root = r.root_words;
        r.root_words = false;
        if (root) r.da.perm = (const uint32_t*)b.hits;
        if ((st = j.mark(4, sk, [&] { return root ? launch_drain_root(r.da, sk) : launch_drain(r.da, mode, sk); })))
            return st;
        if (root) g_root_drain_launches.fetch_add(1);
        r.da.perm = nullptr;
        r.da.count_queue = 0;
        j.drain_launches++;
        r.cur = nx;
        r.live = false;
        return SPT_OK;
    }
    const bool lockstep = it == 0 && r.lock0;
    if (lockstep) j.slot.rs.lockstep_casts += r.known;
    // sharded survivors (spt_internal.h kShards): when the camera cast
    // holds the sub-wavefront's every path and the drain takes the
    // queue next, its per-XCD pools over the same segments
    bool sharded = false;
    if (lockstep && pl.cam_cast) {
        // the first cast, camera ray to shade, in one launch; survivors
        // into queue nx (surv[nx] zeroed with the counters), the
        // refill below keeps the books as after a shade
        sharded = pl.cam_shards && !pl.drain_sort && j.forced_at(r, it + 1);
        CameraCastArgs ca;
        ca.entry = j.entry;
        ca.r = r.ra;  // the first refill's work items (cursor_init: the share's start)
        ca.s = r.sa;
        ca.s.in = r.q[c];
        ca.s.out = r.q[nx];
        ca.s.hits = nullptr;
        ca.s.count_in = &b.cnt->qn[c];
        ca.s.count_out = sharded ? &b.cnt->surv_shard[0][0] : &b.cnt->surv[nx];
        ca.s.shard_items = sharded ? r.known : 0u;
        ca.n = r.known;
        // the bounce cull (an empty scene has no root to visit, and no hit to bounce from)
        unsigned long long* const culled = pl.bounce_cull && !ca.s.sc.empty ? &j.slot.dev->culled[0][0] : nullptr;
        // the root hand-off: this cast is followed at once by the sharded drain
        // of a cached queue.  The hit records are idle on this path (16 B per
        // slot); a survivor's word goes to the slot of its queue entry, and the
        // shards' segments together are the cast's r.known <= cap slots
        r.root_words = sharded && culled && pl.root_handoff && !r.da.nt;
        if (r.root_words) {
            assert((uint64_t)shard_base(kShards, r.known, kIsectBlock) * sizeof(uint32_t) <= kHitBytes * (uint64_t)b.cap);
            ca.s.hits = (const float4*)b.hits;
        }
        if ((st = j.mark(1, sk, [&] { return launch_camera_cast(ca, mode, sk, culled); }))) return st;
        if (sharded) {
            r.da.seg_count = &b.cnt->surv_shard[0][0];
            r.da.seg_items = r.known;
            r.da.seg_block = kIsectBlock;
            r.da.xcd_next = &b.cnt->xcd_next[0][0];
        }
    } else if ((st = j.mark(1, sk, [&] {
                   if (lockstep) return launch_isect_lockstep(r.ia, r.known, sk);
                   return pl.trav_stats ? launch_isect_queue_stats(r.ia, r.known, sk)
                                        : launch_isect_queue(r.ia, r.known, sk);
               })))
        return st;
    // surv[nx] was zeroed by the previous refill (surv_clear)
    r.sa.in = r.q[c]; r.sa.out = r.q[nx];
    r.sa.count_in = &b.cnt->qn[c];
    r.sa.count_out = &b.cnt->surv[nx];
    if (!(lockstep && pl.cam_cast) && (st = j.mark(2, sk, [&] { return launch_shade(r.sa, mode, r.known, sk); })))
        return st;
    // (at a chunk's first iteration the count is known exactly: no
    // conditional drain when it cannot be short)
    if (dph && !(it == 0 && r.known >= r.drain_T)) {
        r.da.q = r.q[c];
        r.da.qcount = &b.cnt->qn[c];
        r.da.drain_below = r.drain_T;
        r.da.perm = nullptr;
        if ((st = j.mark(4, sk, [&] { return launch_drain(r.da, mode, sk); }))) return st;
        j.drain_launches++;
    }
    r.ra.q = r.q[nx]; r.ra.surv = &b.cnt->surv[nx]; r.ra.cursor_in = &b.cnt->cursor[c];
    r.ra.cursor_out = &b.cnt->cursor[nx]; r.ra.qn_out = &b.cnt->qn[nx];
    r.ra.surv_clear = &b.cnt->surv[c];
    r.ra.casts_in = &b.cnt->qn[c];
    r.ra.iter_tag = (uint32_t)it + 2;
    // (after a sharded camera cast: its survivors are the shards' sum, and
    // the drain's per-XCD pool counters start at zero)
    uint32_t* const xcd_keep = r.ra.xcd_next;
    if (sharded) {
        r.ra.surv_shards = &b.cnt->surv_shard[0][0];
        r.ra.xcd_next = &b.cnt->xcd_next[0][0];
    }
    // new paths: at most the work not yet known to be started (one
    // block still runs to carry the counters over)
    const uint32_t fill = (uint32_t)std::min<uint64_t>(b.cap, r.sub_end - r.started);
    // a sharded queue goes to the forced drain next (forced_at): no new path may enter it
    assert(!sharded || fill == 0);
    if ((st = j.mark(0, sk, [&] { return launch_refill(r.ra, fill, sk); }))) return st;
    r.ra.surv_shards = nullptr;
    r.ra.xcd_next = xcd_keep;
    r.cur = nx;
    return SPT_OK;
}

// After a batch of iterations: the unbounded sub-wavefronts' counters are
// copied to snapshot `snap`, and the snapshot queued one batch earlier is
// read (the host lags the launches by a batch and never waits for the newest).
spt_status read_back(RenderJob& j, SubRun* runs, int snap, uint64_t it, int* nlive) {
    const int K = j.pl.K;
    for (int k = 0; k < K; k++) {
        SubRun& r = runs[k];
        if (!r.live || r.limit != UINT64_MAX) continue;  // bounded streams need no readback
        Sub& b = j.ws.sub[k];
        HIP_TRY(hipMemcpyAsync(b.host_cnt + snap, b.cnt, sizeof(Counters), hipMemcpyDeviceToHost, b.stream));
        HIP_TRY(hipEventRecord(b.count_ev[snap], b.stream));
    }
    for (int k = 0; k < K; k++) {
        SubRun& r = runs[k];
        if (!r.live || r.limit != UINT64_MAX) continue;
        Sub& b = j.ws.sub[k];
        if (r.pending >= 0) {
            HIP_TRY(hipEventSynchronize(b.count_ev[r.pending]));
            const Counters& hc = b.host_cnt[r.pending];
            r.known = hc.qn[r.pend_cur];
            r.started = std::max<uint64_t>(r.started, hc.cursor[r.pend_cur]);
            if (r.known == 0) {
                r.live = false;
                (*nlive)--;
                continue;
            }
            // the refill after iteration T - 2 (tag T) started the last
            // work item: its paths cast in iterations T - 1 .. T + max_depth - 2
            if (hc.exhausted) r.limit = hc.exhausted - 1 + j.p.max_depth;
            else if (r.started >= r.sub_end) r.limit = r.pend_it + j.p.max_depth;
        }
        r.pending = snap;
        r.pend_cur = r.cur;
        r.pend_it = it;
    }
    return SPT_OK;
}

// One sample chunk [s0, s0 + ns) on the wavefront: fork, first refill, the
// batched iterations with the lagging readback, join and resolve.
spt_status enqueue_wavefront_chunk(RenderJob& j, SubRun* runs, uint32_t s0, uint32_t ns, uint64_t* iters) {
    WorkSet& ws = j.ws;
    const int K = j.pl.K;
    const hipStream_t stream = j.stream;
    spt_status st;
    HIP_TRY(j.clear_film(ns));
    // fork: the sub-wavefront streams start after everything queued so far
    HIP_TRY(hipEventRecord(ws.fork_ev, stream));
    for (int k = 1; k < K; k++) HIP_TRY(hipStreamWaitEvent(ws.sub[k].stream, ws.fork_ev, 0));
    for (int k = 0; k < K; k++)
        if ((st = first_refill(j, runs[k], k, s0, ns))) return st;
    // isect -> shade -> refill per sub-wavefront until every queue drains.
    // A path cast in iteration i was started by the refill after iteration
    // <= i - 1 and makes at most max_depth casts, so once every work item
    // has been started (the cursor, read back one batch behind the
    // launches, reached the end) the queue is empty max_depth iterations
    // later: the loop stops there without a further readback.  Live counts
    // never grow after that, so a stale count is a safe grid size, and a
    // refill's grid is bounded by the work not yet known to be started.
    const uint64_t L = (uint64_t)ns * j.A;
    const uint64_t max_iters = (L * j.p.max_depth + j.pl.Ck - 1) / j.pl.Ck + j.p.max_depth + 64;
    uint64_t it = 0;
    const uint32_t batch = 4;
    uint32_t nbatch = 0;
    int nlive = 0;
    for (int k = 0; k < K; k++) nlive += runs[k].live ? 1 : 0;
    while (nlive > 0) {
        for (uint32_t bi = 0; bi < batch && nlive > 0; bi++) {
            for (int k = 0; k < K; k++) {
                if (!runs[k].live) continue;
                if ((st = run_iteration(j, runs[k], k, it))) return st;
                if (!runs[k].live) nlive--;
            }
            it++;
        }
        if (nlive == 0) break;
        if ((st = read_back(j, runs, (int)(nbatch++ & 1u), it, &nlive))) return st;
        if (it > max_iters)
            return fail(SPT_ERR_HIP, "spt_render: queue did not drain after %llu iterations", (unsigned long long)it);
        // the batch stays short: the first readback that shows the last work
        // item started bounds the loop, and a long batch would overshoot it
        // (the GPU still has one batch queued while the host waits)
    }
    *iters += it;
    // join the sub-wavefront streams back into the caller's stream
    for (int k = 1; k < K; k++) {
        HIP_TRY(hipEventRecord(ws.sub[k].join_ev, ws.sub[k].stream));
        HIP_TRY(hipStreamWaitEvent(stream, ws.sub[k].join_ev, 0));
    }
    return j.mark(3, stream, [&] { return j.resolve(s0, ns); });
}

// The set's camera entry table for this render's view (RenderPlan::camera_entry;
// the buffer: ensure_workspace), built on `stream` — after the set's previous
// render, before this one's first fork — unless the set holds the table of the
// same geometry, camera, image and tile already.
spt_status ensure_entry(const spt_scene_t* sc, const spt_render_params& p, uint64_t P, const Camera& cam, WorkSet& ws,
                        hipStream_t stream) {
    EntryKey key;
    memset(&key, 0, sizeof(key));  // (compared bytewise: the padding too)
    key.geom_epoch = sc->geom_epoch;
    key.nodes = sc->nodes8;
    key.group_shift = sc->group_shift;
    key.camera = p.camera;
    key.width = p.width; key.height = p.height;
    key.tile_index = p.tile_index; key.tile_count = p.tile_count; key.rows_per_group = p.rows_per_group;
    if (ws.entry_valid && memcmp(&key, &ws.entry_key, sizeof(key)) == 0) return SPT_OK;
    assert(P <= ws.entry_cap);
    ws.entry_valid = false;
    CameraEntryArgs a{};
    a.nodes = sc->nodes8;
    a.group_shift = sc->group_shift;
    a.nslots = (uint32_t)std::min<uint64_t>(sc->node_bytes / (kNode6Quads * 16), 0xffffffffull);
    a.cam = cam;
    a.P = (uint32_t)P; a.W = p.width;
    a.tile_index = p.tile_index; a.tile_count = p.tile_count; a.rows_per_group = p.rows_per_group;
    a.entry = ws.entry;
    HIP_TRY(launch_camera_entry(a, stream));
    ws.entry_key = key;
    ws.entry_valid = true;
    g_entry_builds.fetch_add(1);
    return SPT_OK;
}

// The plan of this render and a working set that holds it: plan_render, then
// ensure_workspace; a set that could not be allocated frees its queues and
// the plan is made again with half the paths in flight as the limit.
spt_status plan_and_allocate(spt_scene_t* sc, const spt_render_params& p, uint64_t P, uint64_t A, hipStream_t caller,
                             spt_render_stats& rs, RenderPlan* plan, WorkSet** set) {
    const spt_config& cfg = sc->cfg;
    for (uint64_t fit_limit = UINT64_MAX;;) {
        const RenderPlanIn in = plan_inputs(sc, p, P, A, caller);
        const RenderPlan pl = plan_render(in, fit_limit);
        rs.fit_paths = pl.fit_paths;
        if (pl.limit)
            return fail(SPT_ERR_LIMIT, "spt_render: wavefront of %llu paths exceeds 2^31", (unsigned long long)pl.C);
        rs.paths_in_flight = (uint32_t)pl.C;
        WorkSet& ws = sc->ws.pick_set(caller);
        ws.last_ticket = sc->ws.next_ticket;
        spt_status st = ensure_workspace(ws, pl.K, pl.Ck, cfg.plane_pad, in.planes, (size_t)pl.chunk * in.film_unit * P,
                                         3 * P, pl.own_queues, pl.sort_buffers, (size_t)(pl.entry_bytes / sizeof(uint32_t)));
        if (st == SPT_ERR_OOM && !pl.fused && pl.C > kMinRetryPaths) {
            // the fit, or below it the per-cast wavefront and its film chunk, halved;
            // first the queues, hit records and film chunk this attempt allocated
            // (ensure_workspace only grows them) are freed, so the halved attempt
            // holds half, not more
            (void)hipGetLastError();
            if ((st = release_queues(ws))) return st;
            rs.fit_retries++;
            fit_limit = pl.C / 2;
            continue;
        }
        if (st) return st;
        *plan = pl;
        *set = &ws;
        return SPT_OK;
    }
}

// spt_render_async (accum null: the film is sum / spp, the running sum in the
// working set) and spt_render_accum_async (accum: samples [sample_base,
// sample_base + spp) added onto the caller's sums) — one render loop; the two
// differ in where the jump table is read and in the resolve.
// With `list` (spt_render_accum_list): the pass over the listed pixels; the
// list is checked on the device first, and the caller's stream waited for.
spt_status render_enqueue(spt_scene sc, const spt_render_params* pp, float* film_dev, const spt_accum* accum,
                          bool accum_call, void* caller_, uint64_t* ticket_out, const spt_pixel_list* list = nullptr,
                          bool list_call = false) {
    const double wall0 = now_ms();
    uint32_t rows = 0;
    spt_status st = check_render_args(sc, pp, film_dev, accum, accum_call, ticket_out, &rows, list, list_call);
    if (st) return st;
    const spt_render_params& p = *pp;
    // The caller's stream orders the render with the caller's work (it starts
    // after what was queued there, and what is queued there next waits for
    // it); the render itself runs on its working set's own streams.
    const hipStream_t caller = (hipStream_t)caller_;
    const uint64_t P = (uint64_t)rows * p.width;
    const uint32_t sample_base = accum ? accum->sample_base : 0u;
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lock(sc->mu);  // the scene's one workspace
    // light sampling lives in the fused lane loop only: refused
    // before any device work rather than rendered with another estimator
    if (sc->lights && (p.flags & (SPT_FLAG_WAVEFRONT | SPT_FLAG_TRAVERSAL_STATS)))
        return fail(SPT_ERR_INVALID, "spt_render: SPT_FLAG_WAVEFRONT / SPT_FLAG_TRAVERSAL_STATS on a scene with light "
                    "sampling on (it runs in the fused pipeline only; spt_scene_set_light_sampling(scene, 0) first)");
    if (sc->sky && (p.flags & (SPT_FLAG_WAVEFRONT | SPT_FLAG_TRAVERSAL_STATS)))
        return fail(SPT_ERR_INVALID, "spt_render: SPT_FLAG_WAVEFRONT / SPT_FLAG_TRAVERSAL_STATS on a scene with sky "
                    "sampling on (it runs in the fused pipeline only; spt_scene_set_sky_sampling(scene, 0, 0.5f) first)");
    RenderSlot* slot = nullptr;
    if ((st = render_slot(sc->ws, &slot))) return st;
    spt_render_stats& rs = slot->rs;
    rs.tile_rows = rows;
    slot->wall0 = wall0;
    if (P == 0 || (list_call && list->n == 0)) {  // an empty tile or list: nothing to render, film untouched
        slot->empty = true;
        slot->ticket = sc->ws.next_ticket++;
        slot->pending = true;
        *ticket_out = slot->ticket;
        return SPT_OK;
    }
    if (list_call) {
        // strictly ascending and in range, or nothing is written
        Workspace& w = sc->ws;
        if (!w.list_bad) HIP_TRY(hipMalloc((void**)&w.list_bad, sizeof(uint32_t)));
        if (!w.list_bad_host) HIP_TRY(hipHostMalloc((void**)&w.list_bad_host, sizeof(uint32_t), hipHostMallocDefault));
        HIP_TRY(hipMemsetAsync(w.list_bad, 0, sizeof(uint32_t), caller));
        HIP_TRY(launch_list_validate(list->pixels, list->n, (uint32_t)P, w.list_bad, caller));
        HIP_TRY(hipMemcpyAsync(w.list_bad_host, w.list_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, caller));
        HIP_TRY(hipStreamSynchronize(caller));
        if (*w.list_bad_host)
            return fail(SPT_ERR_INVALID, "spt_render_accum_list: pixels must be strictly ascending and < %llu",
                        (unsigned long long)P);
    }
    const uint64_t A = list_call ? list->n : 0;  // 0: every tile pixel
    RenderPlan pl;
    WorkSet* set = nullptr;
    if ((st = plan_and_allocate(sc, p, P, A, caller, rs, &pl, &set))) return st;
    WorkSet& ws = *set;
    const int K = pl.K;
    // the set's stream 0 (its own): the render's first and last launches, the
    // fork and join of the other sub-wavefronts
    const hipStream_t stream = ws.sub[0].stream;
    HIP_TRY(hipEventRecord(ws.call_ev, caller));
    HIP_TRY(hipStreamWaitEvent(stream, ws.call_ev, 0));
    JumpTable* jtab = nullptr;
    if ((st = ensure_jumps(sc->ws, stream, sample_base + p.spp, p.max_depth, p.rng_initstate, &jtab))) return st;
    // A pass runs as the sample chunks [sample_base, sample_base + spp) of a longer
    // render: the kernels take a chunk's first sample (sample0 / chunk_s0), index
    // the table by the absolute sample and key the roulette's hash by it
    // (rr_uniform), so sample s of a pass is sample s of any render
    const int set_idx = (int)(&ws - sc->ws.sets);
    const bool timing = (p.flags & SPT_FLAG_TIMING) != 0;
    RenderJob job{sc, p, pl, ws, *slot, film_dev, accum, P, A ? A : P, list_call ? list : nullptr, sample_base,
                  sample_base + p.spp, jtab->samples(),
                  jtab->casts(), make_camera(p.camera, p.width, p.height), stream, timing,
                  timing && (p.flags & SPT_FLAG_TIMING_ALL) != 0};
    // the set's previous render (another stream, perhaps) must be done with it
    if (ws.used) HIP_TRY(hipStreamWaitEvent(stream, ws.free_ev, 0));
    EnqueueGuard guard{ws, stream, caller, *jtab, set_idx, K};
    HIP_TRY(hipMemsetAsync(slot->dev, 0, sizeof(Stats), stream));
    // the camera entry table, where the camera cast can run (first_refill's lock0) over a tree with a root
    sc->ws.entry_set = -1;
    if (pl.camera_entry && pl.fit && pl.drain_on && sc->ntri != 0 && sc->nodes8 && sc->node_bytes) {
        if ((st = ensure_entry(sc, p, P, job.cam, ws, stream))) return st;
        job.entry = ws.entry;
        sc->ws.entry_set = set_idx;
        sc->ws.entry_n = (uint32_t)P;
    }
    // time origin for the isect launch intervals (their union = isect busy time)
    slot->timing = timing;
    if (timing) {
        hipEvent_t origin_ev = nullptr;
        if ((st = get_event(*slot, 0, &origin_ev))) return st;
        if (!sc->ws.epoch) {
            HIP_TRY(hipEventCreate(&sc->ws.epoch));
            HIP_TRY(hipEventRecord(sc->ws.epoch, stream));
        }
        HIP_TRY(hipEventRecord(origin_ev, stream));
    }
    uint64_t iters = 0;
    uint64_t C = pl.C;
    if (pl.fused) {
        uint32_t lanes = 0;
        if ((st = enqueue_fused(job, &iters, &lanes))) return st;
        C = lanes;
        rs.paths_in_flight = lanes;
    } else {
        SubRun runs[kMaxStreams];
        for (int k = 0; k < K; k++) init_sub_run(runs[k], job, ws.sub[k]);
        for (uint32_t s0 = job.s_begin; s0 < job.s_end; s0 += pl.chunk)
            if ((st = enqueue_wavefront_chunk(job, runs, s0, std::min(pl.chunk, job.s_end - s0), &iters))) return st;
    }
    // pinned destination: a pageable one makes the copy a staged, slower transfer
    HIP_TRY(hipMemcpyAsync(slot->host, slot->dev, sizeof(Stats), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(slot->done, stream));
    HIP_TRY(hipEventRecord(ws.free_ev, stream));  // every sub-stream joined `stream` before the resolve
    HIP_TRY(hipEventRecord(jtab->ev[set_idx], stream));  // this render is done with the jump table
    jtab->ev_used[set_idx] = true;
    HIP_TRY(hipStreamWaitEvent(caller, ws.free_ev, 0));  // the caller's next work sees the film
    ws.used = true;
    guard.armed = false;
    rs.iterations = iters;
    rs.drain_launches = job.drain_launches;
    rs.work_order = pl.pixel_major ? SPT_WORK_PIXEL_MAJOR : SPT_WORK_SAMPLE_MAJOR;
    // the policy that ran: every queue kernel has a non-temporal instance,
    // except the traversal-statistics isect variant (diagnostics)
    rs.queue_cache = pl.fused ? 0u : (pl.queue_nt && !pl.trav_stats ? SPT_QUEUE_CACHE_STREAM : SPT_QUEUE_CACHE_CACHED);
    rs.streams = (uint32_t)K;
    rs.fused = pl.fused ? 1u : 0u;
    rs.drain_refill_idle = !pl.fused && pl.drain_on ? pl.drain_idle : 0u;
    slot->regen_base = std::min<uint64_t>(C, job.A * p.spp);
    slot->ticket = sc->ws.next_ticket++;
    slot->pending = true;
    *ticket_out = slot->ticket;
    return SPT_OK;
}

}  // namespace

extern "C" {

void spt_debug_fail_workspace_alloc(int32_t nth) { g_fail_ws_alloc.store(nth < 0 ? -1 : nth); }
uint64_t spt_debug_root_drain_launches(void) { return g_root_drain_launches.load(); }
uint64_t spt_debug_entry_builds(void) { return g_entry_builds.load(); }

spt_status spt_debug_entry_table(spt_scene sc, uint32_t* out, uint32_t capacity, uint32_t* n_out) {
    if (!sc || !n_out || (capacity && !out)) return fail(SPT_ERR_INVALID, "spt_debug_entry_table: NULL argument");
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lock(sc->mu);
    *n_out = 0;
    const int k = sc->ws.entry_set;
    if (k < 0) return SPT_OK;
    const WorkSet& w = sc->ws.sets[k];
    if (!w.entry || !w.entry_valid || sc->ws.entry_n > w.entry_cap) return SPT_OK;
    if (w.used && w.free_ev) HIP_TRY(hipEventSynchronize(w.free_ev));
    const uint32_t n = std::min(capacity, sc->ws.entry_n);
    if (n) HIP_TRY(hipMemcpy(out, w.entry, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    *n_out = sc->ws.entry_n;
    return SPT_OK;
}

spt_status spt_render_async(spt_scene sc, const spt_render_params* pp, float* film_dev, void* caller,
                            uint64_t* ticket_out) {
    return render_enqueue(sc, pp, film_dev, nullptr, false, caller, ticket_out);
}

spt_status spt_render_accum_async(spt_scene sc, const spt_render_params* pp, const spt_accum* acc, void* caller,
                                  uint64_t* ticket_out) {
    return render_enqueue(sc, pp, nullptr, acc, true, caller, ticket_out);
}

spt_status spt_render_accum(spt_scene sc, const spt_render_params* pp, const spt_accum* acc,
                            spt_render_stats* stats_out, void* stream) {
    uint64_t ticket = 0;
    spt_status st = spt_render_accum_async(sc, pp, acc, stream, &ticket);
    if (st) return st;
    return spt_render_wait(sc, ticket, stats_out);
}

spt_status spt_render_accum_list(spt_scene sc, const spt_render_params* pp, const spt_accum* acc,
                                 const spt_pixel_list* list, spt_render_stats* stats_out, void* stream) {
    uint64_t ticket = 0;
    spt_status st = render_enqueue(sc, pp, nullptr, acc, true, stream, &ticket, list, true);
    if (st) return st;
    return spt_render_wait(sc, ticket, stats_out);
}

spt_status spt_render_wait(spt_scene sc, uint64_t ticket, spt_render_stats* stats_out) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_render_wait: NULL scene");
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lock(sc->mu);
    RenderSlot& r = sc->ws.slots[ticket % kRenderSlots];
    if (!r.pending || r.ticket != ticket)
        return fail(SPT_ERR_INVALID, "spt_render_wait: ticket %llu is not a queued render (already collected, "
                    "or %d renders were queued after it)", (unsigned long long)ticket, kRenderSlots);
    return render_collect(r, sc->ws, stats_out);
}

spt_status spt_scene_get_shadow_casts(spt_scene sc, uint64_t* out) {
    if (!sc || !out) return fail(SPT_ERR_INVALID, "spt_scene_get_shadow_casts: NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    *out = sc->ws.last_shadow_casts;
    return SPT_OK;
}

spt_status spt_render(spt_scene sc, const spt_render_params* pp, float* film_dev, spt_render_stats* stats_out,
                      void* stream) {
    uint64_t ticket = 0;
    spt_status st = spt_render_async(sc, pp, film_dev, stream, &ticket);
    if (st) return st;
    return spt_render_wait(sc, ticket, stats_out);
}

spt_status spt_scene_isect_busy_begin(spt_scene sc) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_scene_isect_busy_begin: NULL scene");
    std::lock_guard<std::mutex> lock(sc->mu);
    for (auto& v : sc->ws.iv_all) v.clear();
    sc->ws.collect_iv = true;
    return SPT_OK;
}

spt_status spt_scene_kernel_busy(spt_scene sc, uint32_t kernels, double* busy_ms, uint64_t* launches) {
    if (!sc || !busy_ms) return fail(SPT_ERR_INVALID, "spt_scene_kernel_busy: NULL argument");
    if (kernels == 0 || kernels > (SPT_KERNEL_ISECT | SPT_KERNEL_DRAIN))
        return fail(SPT_ERR_INVALID, "spt_scene_kernel_busy: kernels must be a non-empty mask of SPT_KERNEL_*");
    std::lock_guard<std::mutex> lock(sc->mu);
    std::vector<std::pair<double, double>> iv;
    if (kernels & SPT_KERNEL_ISECT) iv.insert(iv.end(), sc->ws.iv_all[0].begin(), sc->ws.iv_all[0].end());
    if (kernels & SPT_KERNEL_DRAIN) iv.insert(iv.end(), sc->ws.iv_all[1].begin(), sc->ws.iv_all[1].end());
    std::sort(iv.begin(), iv.end());
    *busy_ms = interval_union(iv);
    if (launches) *launches = iv.size();
    return SPT_OK;
}

spt_status spt_scene_isect_busy_end(spt_scene sc, double* busy_ms, uint64_t* launches) {
    if (!sc || !busy_ms) return fail(SPT_ERR_INVALID, "spt_scene_isect_busy_end: NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    std::vector<std::pair<double, double>> iv;
    iv.swap(sc->ws.iv_all[0]);
    sc->ws.iv_all[1].clear();
    sc->ws.collect_iv = false;
    std::sort(iv.begin(), iv.end());
    *busy_ms = interval_union(iv);
    if (launches) *launches = iv.size();
    return SPT_OK;
}

spt_status spt_render_aov(spt_scene sc, const spt_render_params* pp, const spt_aov* out, void* stream_) {
    if (!sc || !pp || !out) return fail(SPT_ERR_INVALID, "spt_render_aov: NULL argument");
    const spt_render_params& p = *pp;
    // spt_render's checks
    if (p.width == 0 || p.height == 0 || p.spp == 0 || p.max_depth == 0)
        return fail(SPT_ERR_INVALID, "spt_render_aov: width/height/spp/max_depth must be > 0");
    if (p.max_depth > kMaxDepthCasts)
        return fail(SPT_ERR_LIMIT, "spt_render_aov: max_depth %u > %u", p.max_depth, kMaxDepthCasts);
    if (p.spp >= (1u << 24)) return fail(SPT_ERR_LIMIT, "spt_render_aov: spp must be < 2^24");
    if ((uint64_t)p.width * p.height >= (1ull << 31)) return fail(SPT_ERR_LIMIT, "spt_render_aov: image too large");
    if (p.tile_count == 0 || p.rows_per_group == 0 || p.tile_index >= p.tile_count)
        return fail(SPT_ERR_INVALID, "spt_render_aov: bad tile (%u of %u, %u rows/group)", p.tile_index, p.tile_count,
                    p.rows_per_group);
    if (p.rng_order > 1) return fail(SPT_ERR_INVALID, "spt_render_aov: rng_order must be 0 or 1");
    if (!out->albedo_r && !out->albedo_g && !out->albedo_b && !out->normal_x && !out->normal_y && !out->normal_z &&
        !out->depth && !out->coverage)
        return fail(SPT_ERR_INVALID, "spt_render_aov: every plane is NULL");
    const hipStream_t stream = (hipStream_t)stream_;
    const uint32_t rows = spt_tile_rows(p.height, p.tile_index, p.tile_count, p.rows_per_group, nullptr, 0);
    AovArgs a;
    a.P = rows * p.width;
    if (a.P == 0) return SPT_OK;  // an empty tile: nothing to write
    a.W = p.width;
    a.spp = p.spp;
    a.rng_order = p.rng_order;
    a.tile_index = p.tile_index; a.tile_count = p.tile_count; a.rows_per_group = p.rows_per_group;
    a.cam = make_camera(p.camera, p.width, p.height);
    a.albedo_r = out->albedo_r; a.albedo_g = out->albedo_g; a.albedo_b = out->albedo_b;
    a.normal_x = out->normal_x; a.normal_y = out->normal_y; a.normal_z = out->normal_z;
    a.depth = out->depth; a.coverage = out->coverage;
    // as spt_intersect: a snapshot of the device arrays, launched and recorded
    // under the mutex (the setters wait for the launch, quiesce_scene)
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lock(sc->mu);
    a.sc = sc->dev();
    // the render's own table: the sample jumps depend on max_depth (4 + 2D draws per sample)
    JumpTable* jtab = nullptr;
    spt_status st = ensure_jumps(sc->ws, stream, p.spp, p.max_depth, p.rng_initstate, &jtab);
    if (st) return st;
    a.sample_jump = jtab->samples();
    if (!jtab->aov_ev) HIP_TRY(hipEventCreateWithFlags(&jtab->aov_ev, hipEventDisableTiming));
    if (jtab->aov_used && jtab->aov_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, jtab->aov_ev, 0));
    HIP_TRY(launch_aov(a, stream));
    HIP_TRY(hipEventRecord(jtab->aov_ev, stream));
    jtab->aov_stream = stream;
    jtab->aov_used = true;
    return record_public_use(sc, stream);
}

}  // extern "C"
