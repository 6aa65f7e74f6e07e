// api_internal.h — what the host files of libdsdtm_amd.so share: the context and the few functions one host file calls in
// another (namespace dsdtm::detail). api.cpp holds every stage but local BA (api_local_ba.cpp); a stage that moves into a file
// of its own brings the names it needs here. Everything else is `static` in its own file. Not included by any kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
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

// The pinned staging block and the device one, each grown to `bytes` (never shrunk)
int ensure_stage(dsdtm_ctx* ctx, size_t bytes);

}  // namespace detail
}  // namespace dsdtm
