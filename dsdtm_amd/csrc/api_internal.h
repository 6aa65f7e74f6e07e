// api_internal.h — what the host files of libdsdtm_amd.so share: the context and the few functions one host file calls in
// another (namespace dsdtm::detail), the small types they pass and the per-call helpers (inline). api.cpp holds every stage but the
// tracked-frame entries (api_track.cpp) and local BA (api_local_ba.cpp); a stage that moves into a file of its own brings the names
// it needs here. What one file alone uses is `static` there. Not included by any kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dsdtm_amd.h"
#include "kernels.h"

struct dsdtm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    char err[512] = {0};
    // staging
    void* h_pinned = nullptr;
    size_t h_cap = 0;
    void* d_stage = nullptr;
    size_t d_cap = 0;
    // workspace for the generic sparse-align kernel
    void* d_ws = nullptr;
    size_t ws_cap = 0;
    // Pair counters of the persistent sparse-align kernel (a launch's slots pull pair indices from one word; the
    // word is zero when a launch starts and the launch's last claim puts it back to zero). A word must never be
    // shared by two launches that can run at the same time, so:
    //  * every stream that launches through this context owns a ring of COUNTERS_PER_STREAM words (a stream runs
    //    its launches in order, so the previous user of a word has finished when the next one starts);
    //  * a launch captured into a hipGraph gets a word of its own from the graph pool, for the life of the
    //    context, and a memset node in front of it (a hipGraphExec never overlaps itself).
    unsigned* d_counter = nullptr;
    // + the stream's workspace, and an event recorded behind the entry's last launch: what a 17th stream waits for
    // before it takes the entry over (the old stream itself may be gone by then)
    struct StreamRing { hipStream_t stream; unsigned seq; bool used; void* d_ws; size_t ws_cap; unsigned long long last_use; hipEvent_t last; bool last_recorded; };
    unsigned long long ring_tick = 0;
    static constexpr int MAX_STREAMS = 16, COUNTERS_PER_STREAM = 8, GRAPH_COUNTERS = 256;
    StreamRing rings[MAX_STREAMS] = {};
    int graph_counters_used = 0;
    // Exchange buffers of the team kernel: a ring of 8 launches x 64 pairs. Team launches of one context are
    // totally ordered (a launch on another stream first waits for the previous team launch's event), because the
    // members of a team spin on each other and must all be resident at once.
    uint8_t* d_team = nullptr;
    unsigned team_seq = 0;
    unsigned long long team_wraps = 0;    // times the 20-bit launch epoch of the exchange tags wrapped (ring re-zeroed each time)
    hipEvent_t team_event = nullptr;      // recorded behind the last team launch that ran on a caller's stream
    hipStream_t team_last_stream = nullptr;
    bool team_any = false;
    // Hand-over timeout words: host-mapped pinned memory of THIS context (a wave whose bounded wait ran out stores 1;
    // the host reads the word once the launch's stream has drained — no copy, no device-global state):
    //   [0, MAX_STREAMS)            one per stream ring: the one-CU launches of that stream
    //   FLAG_GRAPH                  launches captured into hipGraphs
    //   FLAG_SINGLE                 the synchronous single-pair entry points
    //   FLAG_RECOVER + slot         one per multi-CU launch (team / two-member kernels) that has not been settled yet
    static constexpr int RECOVER_SLOTS = 64;
    static constexpr int FLAG_GRAPH = MAX_STREAMS, FLAG_SINGLE = MAX_STREAMS + 1, FLAG_RECOVER = MAX_STREAMS + 2,
                         N_FLAGS = FLAG_RECOVER + RECOVER_SLOTS;
    volatile unsigned* h_flags = nullptr;
    unsigned* d_flags = nullptr;
    // Multi-CU launches wait on partner workgroups, i.e. on the GPU's dispatch: a wait that runs out (a foreign load on
    // the device, another partition mode) must not fail the caller. Every such launch leaves what a re-run needs —
    // descriptor, a copy of its seed poses, an event — and is settled by dsdtm_sparse_align_check (or when its slot is
    // needed again): timeout word clear -> forgotten; set -> poses re-seeded, the same batch relaunched on the one-CU
    // kernels, which cannot wait for anything outside their own workgroup.
    struct Recover {
        bool used = false;
        dsdtm_batch_desc b; dsdtm_camera cam; dsdtm_align_params prm;
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        void* d_seed = nullptr; size_t seed_cap = 0;
        unsigned long long order = 0;
    };
    Recover rec[RECOVER_SLOTS];
    unsigned long long rec_tick = 0;
    unsigned long long recovered = 0;     // launches re-run on the one-CU kernels so far (dsdtm_debug_recovered_launches)
    bool evicted_timeout = false;         // a stream ring was handed to another stream while its timeout word was set
    bool multi_cu_ok = true;              // the dispatch assumptions of the multi-CU kernels hold on this device
    // dsdtm_sparse_align_batch_streamed: two copy streams and one event per chunk, created on first use
    hipStream_t copy_stream[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> copy_events;
    hipEvent_t copy_fence = nullptr;
    int num_cus = 256;
    // Pyramid buffers of destroyed frames, kept for the next frame of the same size: a live tracker creates and destroys one
    // frame per image, and hipMalloc / hipFree (which waits for the whole device) cost more than the pyramid kernel.
    // dsdtm_local_ba*: the descriptors (pinned + device) and the workspace of the local-BA launches, and an event behind the
    // last one (the next launch of this context waits for it before it reuses them)
    void* d_lba = nullptr; size_t lba_cap = 0;
    void* h_lba = nullptr; size_t h_lba_cap = 0;
    hipEvent_t lba_event = nullptr; bool lba_recorded = false;
    hipEvent_t track_event = nullptr;     // dsdtm_track_frame: the local map has arrived (copied up on copy_stream[0] beside Run)
    // dsdtm_frame_prefetch: a stream of its own, created on first use. Prefetched frames are numbered in the order they were
    // enqueued on it; the stream runs in order, so "frame n is resident" implies every earlier one is. Event n % PREFETCH_EVENTS
    // is recorded behind frame n (a wait on an event that a later frame has re-recorded waits a little longer, never too
    // short). The ring is as long as two full batches of dsdtm_track_frames: with step k + 1 of 1024 trackers prefetched before
    // step k is tracked, the event behind step k's last frame is still its own, and the call does not wait for step k + 1.
    // An event is created when its place in the ring is first used. prefetch_settled: the highest number the HOST knows to be resident — frames up to it cost nothing more;
    // prefetch_waiting: the highest number the context's stream has been told to wait for (hipStreamWaitEvent) — it becomes
    // prefetch_settled at the next host synchronisation of that stream.
    static constexpr int PREFETCH_EVENTS = 4096;
    hipStream_t prefetch_stream = nullptr;
    hipEvent_t prefetch_event[PREFETCH_EVENTS] = {};
    unsigned long long prefetch_seq = 0, prefetch_settled = 0, prefetch_waiting = 0;
    // its own pinned staging ring (the context's staging block is busy with frame k while frame k + 1 is staged): a slot
    // is written again only after the frame that used it last is resident
    struct PrefetchSlot { void* h; size_t cap; unsigned long long seq; };
    PrefetchSlot prefetch_slot[2] = {};
    unsigned prefetch_next_slot = 0;
    // (seq: the prefetch number of the destroyed frame — a buffer may go to the pool while its frame is still pending, and
    // its next user's stream then waits for that frame's event, see frame_alloc)
    struct PooledFrame { size_t pitch; uint8_t* d; unsigned long long seq; };
    static constexpr size_t FRAME_POOL = 8;
    std::vector<PooledFrame> frame_pool;
};

namespace dsdtm {
namespace detail {

// The message dsdtm_last_error answers with: the context's, or (ctx NULL) the calling thread's failed dsdtm_create
void set_err(dsdtm_ctx* ctx, const char* fmt, ...);

#define HIP_TRY(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            ::dsdtm::detail::set_err(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return DSDTM_ERR_HIP;                                                            \
        }                                                                                    \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// HIP_TRY for entries that own something until they succeed: answered by the enclosing `fail` lambda (which waits for what was enqueued and releases it)
#define API_TRY(call)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess) { set_err(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return fail(DSDTM_ERR_HIP); } \
    } while (0)

// A pyramid as it lies on the device: dense rows, every level at a 64-byte aligned offset
struct PackedPyr {
    int levels;
    int w[DSDTM_MAX_LEVELS], h[DSDTM_MAX_LEVELS];
    size_t off[DSDTM_MAX_LEVELS];
    size_t bytes;
};

// How a launch is accounted for (see dsdtm_ctx::h_flags / Recover)
struct LaunchMode {
    bool one_cu = false;        // never a team / two-member kernel (re-runs after a timeout, captured launches)
    bool single = false;        // synchronous single-pair entry: its own timeout word, settled by the caller itself
    int variant = -1;           // >= 0: this register variant, whatever max_features (dsdtm_track_frames: max_features is a stride)
    const uint8_t* const* ref_ptrs = nullptr;   // device table of the pairs' reference pyramids (dsdtm_track_frames)
    const uint8_t* const* cur_ptrs = nullptr;   // ... and of their current pyramids (resident frames; with ref_ptrs only)
};

// The frames of one dsdtm_track_frames call share one allocation (a slab: frame i at i * pitch, so that the batch kernels
// address them as packed pyramids); the slab is released when its last frame is destroyed.
struct FrameSlab {
    dsdtm_ctx* owner;
    int device;
    uint8_t* d;
    size_t bytes;
    std::atomic<int> refs;
};

// How level 0 of a caller's gray image reaches the device (dsdtm_track_frame, dsdtm_track_frames, dsdtm_frame_prefetch):
//   STAGED        packed into pinned memory of the entry's own (the caller does, and sets `dev` to its device alias), then as IN_PLACE
//   IN_PLACE      read by ingest_kernel (pyrdown.hip) at `dev`: contiguous, 16-byte aligned, in this device's memory or in pinned
//                 memory the device can address (a pinned image counts as pinned only when it is contiguous: a strided one is staged)
//   COPY_D2D      a strided or odd-address image in this device's memory: hipMemcpy2DAsync
//   COPY_H2D      a pinned image at an odd address, or one the device cannot address: hipMemcpyAsync
//   OTHER_DEVICE  refused, in each entry's own words; `device`: where the image lives
enum ImageRouteKind { STAGED, IN_PLACE, COPY_D2D, COPY_H2D, OTHER_DEVICE };
struct ImageRoute { ImageRouteKind route; const void* dev; int device; };
// What rides with the first ingest launch of a tracked call: Run's inputs and in/out words, pinned -> device
struct RunRange { const void* src; void* dst; size_t bytes; };

}  // namespace detail
}  // namespace dsdtm

struct dsdtm_frame {
    dsdtm_ctx* owner;    // compared only, never dereferenced through the frame (a frame may outlive its context)
    int device;
    uint8_t* d;          // packed pyramid (the layout of plan_pyramid), its own allocation or a place in `slab`
    size_t pitch;        // of the packed pyramid
    dsdtm::detail::PackedPyr pl;
    dsdtm::detail::FrameSlab* slab = nullptr;
    size_t bytes = 0;    // of its own allocation (the pool's size key): the pyramid and, behind it, the depth plane
    float* depth = nullptr;          // pl.w[0] x pl.h[0] floats, metres (dsdtm_frame_prefetch with a depth map), inside the allocation
    unsigned long long seq = 0;      // dsdtm_frame_prefetch: the frame's number on the prefetch stream; 0: never pending
};
// tests/test_frame_prefetch_gpu.py reads a frame's pyramid back through these first members (it has no public entry to do so):
// a change of their layout must fail here, not there
static_assert(offsetof(dsdtm_frame, owner) == 0 && offsetof(dsdtm_frame, device) == 8 && offsetof(dsdtm_frame, d) == 16 &&
              offsetof(dsdtm_frame, pitch) == 24, "struct dsdtm_frame: update _FrameHead in tests/test_frame_prefetch_gpu.py");

namespace dsdtm {
namespace detail {

// api.cpp defines these; api_track.cpp calls them (ensure_stage: api_local_ba.cpp too)
// The pinned staging block and the device one, each grown to `bytes` (never shrunk)
int ensure_stage(dsdtm_ctx* ctx, size_t bytes);
int pinned_device_ptr(dsdtm_ctx* ctx, uint8_t** p);
void plan_image_pyramid(int width, int height, int levels, PackedPyr* pl, int st[]);
uint8_t* pool_take(dsdtm_ctx* ctx, size_t bytes, unsigned long long* seq);
bool pool_give(dsdtm_ctx* ctx, dsdtm_ctx* owner, int device, uint8_t* d, size_t bytes, unsigned long long seq = 0);
int validate_params(dsdtm_ctx* ctx, const dsdtm_align_params* p, int levels);
int launch_batch(dsdtm_ctx* ctx, const dsdtm_batch_desc* b, const dsdtm_camera* cam, const dsdtm_align_params* prm,
                 void* hip_stream, const LaunchMode& mode, bool* multi_cu_used);
void clear_stream_counters(dsdtm_ctx* ctx, hipStream_t stream);
int frame_alloc(dsdtm_ctx* ctx, const PackedPyr& pl, hipStream_t stream, dsdtm_frame** out, bool with_depth = false);
ImageRoute route_image(dsdtm_ctx* ctx, const void* ptr, int width, int stride, bool clear_unaligned, const int* known_mem = nullptr);
int enqueue_level0(dsdtm_ctx* ctx, const ImageRoute& r, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                   const RunRange* run, hipStream_t stream);

// The per-call helpers: inline, so that a call from another file costs what it cost inside api.cpp

// `rows` rows of row_bytes from one pitch to another (one memcpy where both are dense)
inline void copy_rows(void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t row_bytes, size_t rows) {
    if (dst_stride == row_bytes && src_stride == row_bytes) { memcpy(dst, src, row_bytes * rows); return; }
    for (size_t y = 0; y < rows; ++y) memcpy((uint8_t*)dst + y * dst_stride, (const uint8_t*)src + y * src_stride, row_bytes);
}

// the level table of a batch / image descriptor whose pyramids are packed
template <class Desc>
inline void fill_levels(Desc& b, const PackedPyr& pl) {
    b.levels = pl.levels;
    for (int l = 0; l < pl.levels; ++l) { b.width[l] = pl.w[l]; b.height[l] = pl.h[l]; b.stride[l] = pl.w[l]; b.level_offset[l] = pl.off[l]; }
}
// ... and the first `levels` levels of a packed pyramid as the kernels take them
inline void fill_levels(LevelGeom* lv, const PackedPyr& pl, int levels) {
    for (int l = 0; l < levels; ++l) { lv[l].w = pl.w[l]; lv[l].h = pl.h[l]; lv[l].stride = pl.w[l]; lv[l].off = (uint32_t)pl.off[l]; }
}

// A frame that dsdtm_frame_prefetch handed out may still be on its way: before `stream` reads frames numbered up to `seq`
// it waits for the event behind that number — on the device, never on the host. Nothing to do once the host knows the
// frame to be resident (prefetch_settled), or when the context's stream has already been told to wait that far.
inline int frames_consume(dsdtm_ctx* ctx, unsigned long long seq, hipStream_t stream) {
    if (seq <= ctx->prefetch_settled || stream == ctx->prefetch_stream) return DSDTM_OK;
    if (stream == ctx->stream && seq <= ctx->prefetch_waiting) return DSDTM_OK;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->prefetch_event[seq % dsdtm_ctx::PREFETCH_EVENTS], 0));
    if (stream == ctx->stream) ctx->prefetch_waiting = seq;
    return DSDTM_OK;
}
// behind a host synchronisation of the context's stream: what it was told to wait for has arrived.
// INVARIANT: called only after hipStreamSynchronize(ctx->stream) has returned success — never behind a wait for another
// stream or for an event: prefetch_waiting counts the waits enqueued on ctx->stream alone (frames_consume).
inline void frames_settle(dsdtm_ctx* ctx) {
    if (ctx->prefetch_waiting > ctx->prefetch_settled) ctx->prefetch_settled = ctx->prefetch_waiting;
}

}  // namespace detail
}  // namespace dsdtm
