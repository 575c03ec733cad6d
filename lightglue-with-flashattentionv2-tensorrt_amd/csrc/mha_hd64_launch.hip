// mha_hd64_launch.hip — the attention launcher: fills the kernels' argument tables from the plan of
// mha_hd64_plan.cpp and launches the kernel family it names; owns the arrival tickets of the
// in-launch split combine. No kernel lives here; a .hip only for the argument types of mha_hd64_device.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

#include "mha_hd64_device.h"
#include "mha_hd64_internal.h"

namespace mha_hd64 {

static unsigned long long* g_stamps = nullptr;  // diagnostic builds (MHA_STAMPS) only
void set_stamp_buffer(void* p) { g_stamps = reinterpret_cast<unsigned long long*>(p); }

// ---- arrival tickets of the in-launch combine ----
// Every ticket a launch uses is zero when it starts and zero when it ends (the last arriver of
// each group resets its own), so a ticket array needs no per-call reset as long as no two launches
// that use it run concurrently:
//  * eager launches: one array per (device, stream) -- launches on one stream are serialised;
//  * launches recorded under stream capture: a slice of their own, carved from a per-device arena
//    (an instantiated graph never runs concurrently with itself, while two graphs captured on one
//    stream may be replayed side by side).
// Arrays are created only outside capture (hipMalloc + memset, then a one-time stream sync for the
// arena); a launch that finds no tickets combines in the second kernel instead. Nothing is freed
// (a launch in flight or a graph may still reference it). A half-used arena is replaced at the
// next eager launch (tickets_for), at most kMaxArenas times per device: memory for tickets is
// bounded by (kMaxArenas + 1) x 4 MiB per device plus the per-stream arrays; past the cap, captures
// that find the arena full use the combine kernel (same bits). So an EAGER split launch may
// allocate device memory (never more than that bound); it does so with this thread's capture mode
// exchanged to relaxed, so a global-mode capture running on another thread stays valid.
namespace {
int g_fused = -1;  // -1: unset (env MHA_HD64_FUSED_COMBINE, default on), 0 off, 1 on
std::mutex g_ticket_mu;
std::map<std::pair<int, hipStream_t>, std::pair<unsigned*, int>> g_tickets;
struct Arena {
    unsigned* base = nullptr;
    int cap = 0;
    int used = 0;
    int replaced = 0;
};
std::map<int, Arena> g_arena;
thread_local int g_last_combine = 0;  // this thread's last launch: 0 no split, 1 in-launch, 2 kernel
constexpr int kArenaTickets = 1 << 20;  // 4 MiB per device
constexpr int kMaxArenas = 4;           // replacements per device
// Scoped relaxed capture mode for this thread: allocation calls stay legal (and do not invalidate
// another thread's global-mode capture) while any capture is in progress in the process.
struct RelaxedCapture {
    hipStreamCaptureMode prev = hipStreamCaptureModeRelaxed;
    RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&prev); }
    ~RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&prev); }
};
}  // namespace

int last_combine_form() { return g_last_combine; }

void set_fused_combine(int enable) {
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    g_fused = enable ? 1 : 0;
}

static bool fused_enabled() {
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    if (g_fused < 0) {
        const char* e = std::getenv("MHA_HD64_FUSED_COMBINE");
        g_fused = (e && e[0] == '0') ? 0 : 1;
    }
    return g_fused == 1;
}

static unsigned* zeroed_tickets(int count, hipStream_t stream) {
    unsigned* p = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&p), (size_t)count * sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemsetAsync(p, 0, (size_t)count * sizeof(unsigned), stream) != hipSuccess) {
        (void)hipFree(p);
        return nullptr;
    }
    return p;
}

static unsigned* tickets_for(hipStream_t stream, int count) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    Arena& ar = g_arena[dev];
    if (cs != hipStreamCaptureStatusNone) {  // a slice owned by this recorded launch
        const int n = (count + 63) & ~63;
        if (!ar.base || ar.used + n > ar.cap) return nullptr;
        unsigned* p = ar.base + ar.used;
        ar.used += n;
        return p;
    }
    // First eager launch on this device: the arena for later captures. An arena more than half
    // carved is replaced by a fresh one at the next eager launch (the old one stays allocated: graphs
    // recorded from it may still run), at most kMaxArenas times, so captures run out only after
    // 512 Ki tickets recorded with no eager launch in between.
    RelaxedCapture relaxed;
    if (!ar.base || (ar.used > ar.cap / 2 && ar.replaced < kMaxArenas)) {
        unsigned* fresh = zeroed_tickets(kArenaTickets, stream);
        if (fresh && hipStreamSynchronize(stream) == hipSuccess) {
            if (ar.base) ++ar.replaced;  // (counted only once a fresh arena is installed)
            ar.base = fresh;
            ar.cap = kArenaTickets;
            ar.used = 0;
        } else {
            if (fresh) (void)hipFree(fresh);  // a failed attempt leaks nothing
            if (!ar.base) ar.cap = 0;
        }
    }
    auto& slot = g_tickets[{dev, stream}];
    if (slot.first && slot.second >= count) return slot.first;
    const int cap = std::max(count, 4096);
    unsigned* p = zeroed_tickets(cap, stream);
    if (!p) return nullptr;
    slot = {p, cap};
    return p;
}

// The convert route of an fp32-input launch (route_chunk): the fp16 copies of Q, K, V laid out
// in the workspace call after call, c16 = the calls reading them, and the one convert launch.
static hipError_t convert_to_f16(const Call* calls, int n, Call* c16, void* workspace, hipStream_t stream,
                                 int phase_mask) {
    const void* src[kConvMax];
    void* dst[kConvMax];
    unsigned end8[kConvMax], total8 = 0;
    int count = 0;
    char* ws = reinterpret_cast<char*>(workspace);
    for (int i = 0; i < n; ++i) {
        c16[i] = calls[i];
        if (calls[i].nq <= 0 || calls[i].batch <= 0 || calls[i].heads <= 0) continue;
        const int rows[3] = {calls[i].nq, calls[i].nkv, calls[i].nkv};
        const void* from[3] = {calls[i].q, calls[i].k, calls[i].v};
        const void** to[3] = {&c16[i].q, &c16[i].k, &c16[i].v};
        for (int j = 0; j < 3; ++j) {
            total8 += (unsigned)((size_t)calls[i].batch * calls[i].heads * rows[j] * kHeadDim / 8);
            src[count] = from[j];
            dst[count] = ws;
            end8[count++] = total8;
            *to[j] = ws;
            ws += f16_copy_bytes(calls[i], rows[j]);
        }
    }
    if (total8 == 0 || !(phase_mask & 1)) return hipSuccess;
    return launch_convert(src, dst, end8, count, stream);
}

// lens (the streaming kernel's per-item key counts, launch_group's comment): lens[i] belongs to calls[i]
static hipError_t launch_group_chunk(const Call* calls, int n, InType in, OutType out, void* workspace,
                                     size_t ws_bytes, hipStream_t stream, int force_q_waves, int force_kv_waves,
                                     int force_splits, int phase_mask, const int* const* lens, const int* const* qlens) {
    const ChunkRoute r = route_chunk(calls, n, in, ws_bytes, workspace != nullptr, force_q_waves, force_kv_waves,
                                     force_splits);
    const GroupPlan& p = r.plan;
    Call c16[kMaxCalls];
    if (r.route == Route::F32Convert) {
        const hipError_t e = convert_to_f16(calls, n, c16, workspace, stream, phase_mask);
        if (e != hipSuccess) return e;
        calls = c16;
        in = InType::F16;
        lens = qlens = nullptr;
    }
    FwdArgs a{};
    a.stamps = g_stamps;
    int blocks = 0, n_live = 0;
    bool any_split = false;
    for (int i = 0; i < n; ++i) {
        const Call& c = calls[i];
        if (c.nq <= 0 || c.batch <= 0 || c.heads <= 0) continue;  // nothing to compute
        CallArgs& ca = a.c[n_live];
        ca.q = c.q;
        ca.k = c.k;
        ca.v = c.v;
        ca.o = c.o;
        ca.nq = c.nq;
        ca.nkv = c.nkv;
        ca.splits = p.splits[i];
        ca.tiles_per_split = p.tiles_per_split[i];
        ca.bh = c.batch * c.heads;
        ca.heads = c.heads;
        a.lens[n_live] = lens ? lens[i] : nullptr;
        a.qlens[n_live] = lens && qlens ? qlens[i] : nullptr;
        const int block_m = p.rows_per_wave == 16 ? 16 : 32 * p.q_waves * (p.rows_per_wave / 32);
        ca.qtiles = (c.nq + block_m - 1) / block_m;
        ca.block_begin = blocks;
        if (ca.splits > 1) {
            const size_t rows = (size_t)ca.bh * ca.splits * c.nq;
            char* base = reinterpret_cast<char*>(workspace) + p.ws_offset[i];
            ca.part_o = base;
            ca.part_ml = reinterpret_cast<float2*>(base + align256(rows * kHeadDim * sizeof(float)));
            any_split = true;
        }
        blocks += ca.qtiles * ca.bh * ca.splits;
        ++n_live;
    }
    if (n_live == 0) return hipSuccess;
    a.n_calls = n_live;
    a.total_blocks = blocks;
    const int rbw = p.rows_per_wave / 32;
    if (p.stream) {  // persistent streaming kernel: no split, no workspace
        g_last_combine = 0;
        if (!(phase_mask & 1)) return hipSuccess;
        return launch_stream(a, p.q_waves, out == OutType::F32, stream, lens != nullptr);
    }
    if (lens) return hipErrorInvalidValue;  // (only the streaming kernel takes key counts)
    if (p.direct_tiles > 0) {  // single-pass kernel: no split, no workspace
        g_last_combine = 0;
        if (!(phase_mask & 1)) return hipSuccess;
        return p.rows_per_wave == 16 ? launch_direct16(a, blocks, p.direct_tiles, out == OutType::F32, stream,
                                                       r.route == Route::F32InKernel)
                                     : launch_direct(a, blocks, p.direct_tiles, out == OutType::F32, stream);
    }
    // Split calls combine inside the main launch when a ticket array is available (phase_mask 3,
    // the production form); otherwise (or MHA_HD64_FUSED_COMBINE=0) in the combine kernel.
    if (any_split && (phase_mask & 3) == 3 && fused_enabled()) a.tickets = tickets_for(stream, blocks);
    g_last_combine = !any_split ? 0 : (a.tickets ? 1 : 2);
    hipError_t e = hipSuccess;
    if (phase_mask & 1)
        e = launch_ring(a, blocks, p.q_waves, p.kv_waves, rbw, in == InType::F32, out == OutType::F32, stream);
    if (e != hipSuccess || !any_split || !(phase_mask & 2) || a.tickets) return e;
    return launch_combine(a, 32 * p.q_waves * rbw, out == OutType::F32, stream);
}

hipError_t launch_group(const Call* calls, int n, InType in, OutType out, void* workspace, size_t ws_bytes,
                        hipStream_t stream, int force_q_waves, int force_kv_waves, int force_splits,
                        int phase_mask, const int* const* lens, const int* const* qlens) {
    // Chunks of kMaxCalls calls share one launch; each chunk reuses the workspace (stream order).
    for (int i = 0; i < n; i += kMaxCalls) {
        const hipError_t e = launch_group_chunk(calls + i, std::min(kMaxCalls, n - i), in, out, workspace, ws_bytes,
                                                stream, force_q_waves, force_kv_waves, force_splits, phase_mask,
                                                lens ? lens + i : nullptr, qlens ? qlens + i : nullptr);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_attention(const Call& c, InType in, OutType out, void* workspace, size_t ws_bytes,
                            hipStream_t stream, int force_q_waves, int force_kv_waves, int force_splits,
                            int phase_mask) {
    return launch_group(&c, 1, in, out, workspace, ws_bytes, stream, force_q_waves, force_kv_waves, force_splits,
                        phase_mask);
}

}  // namespace mha_hd64
