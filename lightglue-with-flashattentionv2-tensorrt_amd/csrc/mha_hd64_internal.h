// mha_hd64_internal.h — host-side launch plumbing shared by the kernels and the plugin shim.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace mha_hd64 {

constexpr int kHeadDim = 64;
constexpr int kMaxSeqLen = 2048;
constexpr int kNumHeads = 4;
constexpr int kTileKV = 64;     // keys per LDS tile
constexpr int kMaxSplits = 16;  // KV splits per query group (combine loads them all in one round)

enum class InType { F16, F32 };
enum class OutType { F16, F32 };

// One attention call: Q [batch, heads, nq, 64], K/V [batch, heads, nkv, 64], O like Q.
// Contiguous row-major ("kLINEAR"), the layout the reference plugin receives
// (lightglue_attention_plugin.cpp:122-163, head stride N*64).
struct Call {
    const void* q;
    const void* k;
    const void* v;
    void* o;
    int batch;
    int heads;
    int nq;
    int nkv;
};

// Up to kGroupCalls calls share one launch (grouped launcher); larger groups are chunked.
constexpr int kGroupCalls = 4;

// Plan of one launch carrying n <= kGroupCalls calls: one workgroup shape, per-call KV split,
// per-call workspace offsets (split partials laid out call after call).
struct GroupPlan {
    int q_waves;
    int kv_waves;
    int rows_per_wave;  // 32, or 64 (two query blocks per wave share every K/V fragment read); 16: the 16-row kernel
    int splits[kGroupCalls];           // KV split across workgroups (1 = no combine pass)
    int tiles_per_split[kGroupCalls];  // KV super-tiles (64 * kv_waves keys) per split
    size_t ws_offset[kGroupCalls];
    size_t ws_needed;
    int direct_tiles;  // > 0: the single-pass kernel (mha_hd64_direct.hip), q_waves 1 x kv_waves 8
    int stream;        // 1: the persistent streaming kernel (mha_hd64_stream.hip), 128-row items
};
// force_q_waves = kForceDirect selects the single-pass kernel (fp16 input, nkv <= 1024).
constexpr int kForceDirect = 21;
// force_q_waves = kForceDirect16 selects the 16-row single-pass kernel (mha_hd64_direct16.hip).
constexpr int kForceDirect16 = 22;
// force_q_waves = kForceStream selects the persistent streaming kernel (mha_hd64_stream.hip).
constexpr int kForceStream = 23;
// The plan as the test hooks report and force it: 21 / 22 / 23, or q_waves (+ 10 with 64-row waves).
inline int plan_code(const GroupPlan& p) {
    if (p.stream) return kForceStream;
    if (p.direct_tiles > 0) return p.rows_per_wave == 16 ? kForceDirect16 : kForceDirect;
    return p.q_waves + (p.rows_per_wave == 64 ? 10 : 0);
}
// Workgroup shapes compiled (mha_hd64_ring.hip): (q_waves, kv_waves) in {(4,1), (2,2), (1,2), (4,2),
// (2,4), (1,4), (1,8)} with 32-row waves, and (2,2) with 64-row waves (forced as q_waves = 12).
bool valid_shape(int q_waves, int kv_waves, int row_blocks);
GroupPlan plan_group(const Call* calls, int n, size_t ws_bytes, int force_q_waves = 0, int force_kv_waves = 0,
                     int force_splits = 0, InType in = InType::F16);
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t split_workspace_bytes(const Call& c, int splits);
// Workspace bytes of the fp16 copy of `rows` rows per (batch, head) of call c (the convert route).
inline size_t f16_copy_bytes(const Call& c, int rows) {
    return align256((size_t)c.batch * c.heads * rows * kHeadDim * 2);
}

// How one launch (a chunk of n <= kGroupCalls calls) runs: the planner's plan for its input type,
// or for fp32 inputs one of the two routes onto the fp16 single-pass / streaming kernels.
enum class Route { Planned, F32InKernel, F32Convert };
struct ChunkRoute {
    Route route;
    GroupPlan plan;   // the plan to launch (F32InKernel: the fp16 16-row plan; F32Convert: the fp16 plan)
    size_t ws_bytes;  // workspace the route uses: split partials, or the fp16 copies of Q, K, V
};
// The one routing decision of a launch, shared by the launcher and the workspace query
// (ws_bytes = (size_t)-1 with has_workspace: what the launch would use at best).
ChunkRoute route_chunk(const Call* calls, int n, InType in, size_t ws_bytes, bool has_workspace,
                       int force_q_waves = 0, int force_kv_waves = 0, int force_splits = 0);
// lens (non-null only with force_q_waves = kForceStream and fp16 inputs): lens[i] is a device table of
// calls[i].batch int32 key counts, or null; item b of call i attends to its first lens[i][b] keys
// (clamped into [1, nkv] in the kernel). qlens (with lens only; may be null): the same for query rows
// (qlens[i][b] real rows of item b; the rows past it are written as NaN and influence no other row).
hipError_t launch_group(const Call* calls, int n, InType in, OutType out, void* workspace, size_t ws_bytes,
                        hipStream_t stream, int force_q_waves = 0, int force_kv_waves = 0, int force_splits = 0,
                        int phase_mask = 3, const int* const* lens = nullptr, const int* const* qlens = nullptr);
// Workspace bytes launch_group can use for these calls with inputs of type `in`: the largest
// chunk's need (chunks of kGroupCalls reuse the workspace in stream order) -- split partials, or
// for fp32 inputs the fp16 copies the convert launch writes when a single-pass kernel runs them.
size_t group_workspace_bytes(const Call* calls, int n, InType in = InType::F16);

// Returns hipSuccess or the launch error. phase_mask (measurement hook): bit 0 = main
// kernel, bit 1 = split-KV combine kernel.
hipError_t launch_attention(const Call& c, InType in, OutType out, void* workspace, size_t ws_bytes,
                            hipStream_t stream, int force_q_waves = 0, int force_kv_waves = 0,
                            int force_splits = 0, int phase_mask = 3);

// Record an error for mha_hd64_last_error() (and abort if abort-on-error is set); returns status.
int32_t report_error(int32_t status, const char* where, const char* what);

// Diagnostic builds (-DMHA_STAMPS): where the kernel writes its per-workgroup timestamps.
void set_stamp_buffer(void* p);
// In-launch split combine on/off (default on unless env MHA_HD64_FUSED_COMBINE=0).
void set_fused_combine(int enable);
int set_stream_mode(int mode);      // 1 = persistent streaming kernel for large fp16 launches; returns the previous
void set_f32_inkernel(int enable);  // fp32 inputs: 1 = rounded in the 16-row kernel, 0 = convert launch,
                                    // 2 = also the two-pass forms (diagnostic)
// How the calling thread's last launch merged its splits: 0 none, 1 in-launch, 2 combine kernel.
int last_combine_form();
// Concurrent enqueue streams the host keeps busy (mha_hd64_set_concurrency_hint); >= 1.
int concurrency_hint();
int set_concurrency_hint(int streams);

}  // namespace mha_hd64
