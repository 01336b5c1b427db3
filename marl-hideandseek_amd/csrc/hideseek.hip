// libhideseek.so — host side of the C ABI declared in include/hideseek.h.
// Owns the HBM allocations, launches the two kernels of a step on the handle's HIP stream and
// hands out non-owning tensor descriptors (replaces Manager::Impl, src/mgr.cpp:86-437, 674-822).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <atomic>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <memory>
#include <type_traits>

#include "../../include/hideseek.h"
#include "hs_state.h"
#include "hs_k_reset.h"
#include "hs_k_observe.h"
#include "hs_k_render.h"
#include "hs_k_spectate.h"
#include "hs_k_physics.h"
#include "hs_k_balance.h"
#include "hs_k_pack.h"
#include "hs_k_sample.h"
#include "hs_k_gae.h"
#include "hs_k_ppo.h"
#include "hs_k_twohot.h"
#include "hs_rows.h"
#include "hs_k_embed.h"
#include "hs_k_norm.h"
#include "hs_solver.h"
#include "hs_k_lstm.h"
#include "hs_k_dense.h"
#include "hs_k_gather.h"                  // ahead of hs_k_adam.h: its one kernel is a template, emitted where launch_gather (the last stage) names it
#include "hs_k_episode.h"                 // likewise: its two kernels are templates, emitted where launch_episode (after launch_gather) names them
#include "hs_k_behaviour.h"               // likewise: emitted where launch_behaviour (after launch_attend) names them
#include "hs_k_league.h"                  // likewise: emitted where launch_league (after launch_episode) names them
#include "hs_k_pack_routed.h"             // likewise: emitted where launch_pack_routed (after launch_league) names it
#include "hs_k_sample_routed.h"           // likewise: emitted where launch_sample_routed (after launch_pack_routed) names it
#include "hs_k_attend.h"                  // likewise: emitted where launch_attend (after launch_gae_grouped) names them
#include "hs_k_reduce.h"                  // likewise: emitted where launch_reduce (at the end of this file) names it; it includes hs_k_adam.h itself
#include "hs_k_hash.h"                    // likewise: emitted where launch_hash and launch_hash_bwd (at the end of this file, after launch_reduce) name them
#include "hs_k_loss_scale.h"              // likewise: emitted where launch_adam_scaled (after launch_behaviour) names them; it includes hs_k_adam.h itself
#include "hs_k_adam.h"
#include "hs_core_probe.h"                // after every kernel header: the scalar core's probe table, read by k_core_eval alone

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HS_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(HS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)
#define HS_TRY(expr)                                                                          \
    do {                                                                                      \
        const int rc_ = (expr);                                                               \
        if (rc_ != HS_OK) return rc_;                                                         \
    } while (0)
// How every entry point opens: its arguments are there, and the handle's device is the current one.
#define HS_ENTER(args_ok, msg)                                                                \
    do {                                                                                      \
        if (!(args_ok)) return fail(HS_ERR_INVALID_ARG, msg);                                 \
        HS_HIP(hipSetDevice(s->cfg.gpu_id));                                                  \
    } while (0)

// hs_set_late_threshold: the default (fixed by measurement) and the largest factor kept ("nobody is late")
constexpr float kDefaultLateFactor = 1.00f, kMaxLateFactor = 1.0e6f;

}  // namespace

struct hs_sim {
    hs_config cfg;
    hs::SimState S;
    int A;
    std::vector<void *> allocs;
    hs_tensor_desc exports[HS_NUM_EXPORTS];
    bool profiling = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float last_ms[3] = {0.f, 0.f, 0.f};
    bool initialised = false;
    hipStream_t step_stream = nullptr;     // the stream of the open step
    int step_idx = 0;                      // physics launches mod 3 (SimState::tickSum)
    // Load balancing between the physics waves (hs_k_balance.h): a deal every kBalancePeriod steps
    int steps_since_balance = 0;
    int *bal_hist = nullptr, *bal_cursor = nullptr, *bal_new_slot = nullptr;
    void *bal_tmp = nullptr;               // a second arena: the deal copies the columns there and moves them back to their new slots
    void *col_arena = nullptr; size_t col_arena_bytes = 0, col_slots = 0;      // the tiled columns, one after the other
    hs::BalanceCols bal_cols;              // first arena row of each column (+ the total)
    hipStream_t stream = nullptr;          // this handle's own stream: hs_init / hs_step / checkpoints run here
    hipEvent_t evIn = nullptr;             // orders `stream` after the device's legacy default stream (torch's writes to `action`)
    bool step_open = false;                // hs_step_begin without its hs_step_end
    bool split_fits = false;               // the octets leave physics wave slots free (hs_create): two launches place their waves at once
    bool split_open = false;               // the open step runs split: its early chain is on `stream` (launch_step)
    int64_t split_steps = 0;               // steps run split since hs_create (hs_get_device_status)
    std::atomic<int32_t> async_error{0};   // a failed XLA custom call on this handle (hs_xla_*: the ABI has no status channel; XLA's thread)
    hs::SpectateCam *cams = nullptr;       // hs_render_cameras: the device copy of the cameras, grown on demand
    int cam_cap = 0;
    double *pack_partials = nullptr;       // hs_pack_policy_inputs: the moments of each workgroup, [pack_grid][HS_PACK_MOMENTS]
    double *pack_routed_partials = nullptr;        // hs_pack_policy_inputs_routed: [N][pack_routed_grid][HS_PACK_MOMENTS], N G <= kPackMaxGrid for every N
    double *gae_partials = nullptr;        // hs_compute_gae: the moments of each workgroup, [gae_grid][HS_GAE_MOMENTS]; grouped: [G][gae_grid(R / G)][..]
    double *ppo_partials = nullptr;        // hs_ppo_loss: the statistics of each workgroup, [kPpoMaxGrid][HS_PPO_STATS]
    int32_t *ppo_counts = nullptr;         // hs_ppo_loss: the active samples each workgroup of k_ppo_count saw, [kPpoCountGrid]
    double *twohot_partials = nullptr;     // hs_twohot_value: the statistics of each workgroup, [kTwMaxGrid][HS_TWOHOT_STATS]
    int32_t *twohot_counts = nullptr;      // hs_twohot_value: its own counts of k_ppo_count, [kPpoCountGrid]
    float *embed_partials = nullptr;       // hs_entity_encode_backward: the sums of each workgroup, [kRowsMaxGridBwd][HS_EMBED_PARAM_ROWS * kEmbMaxE]
    float *lstm_partials = nullptr;        // hs_lstm_cell_backward: the sums of each workgroup, [kRowsMaxGridBwd][HS_LSTM_PARAM_ROWS * kLstmMaxH]
    float *hash_partials = nullptr;        // hs_hash_encode_backward: the bins' sums of each workgroup, then their sum, [kHashMaxGridBwd + 1][kHashBins * kHashFeat]
    float *dense_partials = nullptr;       // hs_dense_norm_act_backward: the sums of each workgroup, [kRowsMaxGridBwd][HS_DENSE_PARAM_ROWS * kDenseMaxC]
    double *adam_workspace = nullptr;      // hs_adam_step: the sum of squares of each workgroup and the snapshot of the state, [kAdamWorkspace]; hs_adam_step_scaled: then the snapshot of the loss-scale state, [kLossScaleWorkspace]
    double *episode_partials = nullptr;    // hs_episode_stats: the sums of each workgroup, [episode_grid][HS_EPISODE_STATS]
    double *behaviour_partials = nullptr;  // hs_behaviour_stats: the sums of each workgroup, [behaviour_grid][HS_BEHAVIOUR_STATS]
    int32_t *league_step = nullptr;        // hs_league_step: the counts of the step and its malformed worlds, [kLeagueMaxBins + 1], zero between calls
    int4 *league_table = nullptr;          // hs_league_set_schedule: (hiders, seekers, the sides each holds before the pair), [kLeagueMaxGroup]
    int league_group = 0, league_sides = 0, league_policies = 0;       // the table's G (0: none set), c = 2 G / N, and N

    template <typename T> int dalloc(T **p, size_t n, int fill_byte = 0) {
        void *d = nullptr;
        HS_HIP(hipMalloc(&d, n * sizeof(T) > 0 ? n * sizeof(T) : 4));
        HS_HIP(hipMemset(d, fill_byte, n * sizeof(T) > 0 ? n * sizeof(T) : 4));
        allocs.push_back(d);
        *p = (T *)d;
        return HS_OK;
    }
};

namespace {

// The exported tensors (ExportID, src/sim.hpp:45-68; mgr.cpp:1062-1336), one row per HS_EXPORT_* id in id order: element
// type, rows per world or per agent, trailing dims (0: absent), and the SimState field the kernels reach it through.
// hs_create allocates and describes them from here, and every byte count of a stream copy is that of a descriptor
// (bytes_of).  The two renderer outputs are not rows: their dims come from the config and they are allocated on first need.
struct ExportRow { int32_t id, dtype; bool per_agent; int64_t tail[2]; size_t field; };
static_assert(std::is_standard_layout<hs::SimState>::value, "offsetof(hs::SimState, ...)");
#define HS_X(f) offsetof(hs::SimState, f)
constexpr ExportRow kExports[] = {
    {HS_EXPORT_RESET, HS_DTYPE_I32, false, {1}, HS_X(xReset)},
    {HS_EXPORT_PREP_COUNTER, HS_DTYPE_I32, true, {1}, HS_X(xPrep)},
    {HS_EXPORT_ACTION, HS_DTYPE_I32, true, {5}, HS_X(xAction)},
    {HS_EXPORT_SELF_OBS, HS_DTYPE_F32, true, {13}, HS_X(xSelfObs)},
    {HS_EXPORT_SELF_TYPE, HS_DTYPE_I32, true, {1}, HS_X(xSelfType)},
    {HS_EXPORT_SELF_MASK, HS_DTYPE_F32, true, {1}, HS_X(xSelfMask)},
    {HS_EXPORT_AGENT_OBS, HS_DTYPE_F32, true, {5, 14}, HS_X(xAgentObs)},
    {HS_EXPORT_BOX_OBS, HS_DTYPE_F32, true, {9, 17}, HS_X(xBoxObs)},
    {HS_EXPORT_RAMP_OBS, HS_DTYPE_F32, true, {2, 14}, HS_X(xRampObs)},
    {HS_EXPORT_AGENT_VIS_MASKS, HS_DTYPE_F32, true, {5, 1}, HS_X(xVisAgents)},
    {HS_EXPORT_BOX_VIS_MASKS, HS_DTYPE_F32, true, {9, 1}, HS_X(xVisBoxes)},
    {HS_EXPORT_RAMP_VIS_MASKS, HS_DTYPE_F32, true, {2, 1}, HS_X(xVisRamps)},
    {HS_EXPORT_LIDAR, HS_DTYPE_F32, true, {30}, HS_X(xLidar)},
    {HS_EXPORT_SEED, HS_DTYPE_I32, true, {2}, HS_X(xSeed)},
    {HS_EXPORT_REWARD, HS_DTYPE_F32, true, {1}, HS_X(xReward)},
    {HS_EXPORT_DONE, HS_DTYPE_I32, true, {1}, HS_X(xDone)},
    {HS_EXPORT_GLOBAL_DEBUG_POSITIONS, HS_DTYPE_F32, false, {17, 2}, HS_X(xGlobalPos)},
    {HS_EXPORT_AGENT_POLICY, HS_DTYPE_I32, true, {1}, HS_X(xPolicy)},
    {HS_EXPORT_EPISODE_RESULT, HS_DTYPE_F32, false, {2}, HS_X(xEpisodeResult)},
    // raw bytes, as the reference exports them (mgr.cpp:1209-1227)
    {HS_EXPORT_CHECKPOINT_CONTROL, HS_DTYPE_U8, false, {sizeof(int32_t)}, HS_X(xCkptCtrl)},
    {HS_EXPORT_CHECKPOINT, HS_DTYPE_U8, false, {sizeof(hs_checkpoint)}, HS_X(xCkpt)},
};
#undef HS_X
static_assert(sizeof(kExports) / sizeof(kExports[0]) == HS_EXPORT_DEPTH, "a row per export below the renderer outputs");

// k_pack's row (hs_k_pack.h) is made of these exports, with their widths
constexpr bool pack_table(int id, int64_t t0, int64_t t1, int32_t dtype = HS_DTYPE_F32) {
    return kExports[id].id == id && kExports[id].per_agent && kExports[id].dtype == dtype && kExports[id].tail[0] == t0 && kExports[id].tail[1] == t1;
}
static_assert(pack_table(HS_EXPORT_PREP_COUNTER, 1, 0, HS_DTYPE_I32) && pack_table(HS_EXPORT_SELF_TYPE, 1, 0, HS_DTYPE_I32) &&
              pack_table(HS_EXPORT_SELF_MASK, 1, 0) && pack_table(HS_EXPORT_SELF_OBS, hs::kPackSelfW, 0) &&
              pack_table(HS_EXPORT_LIDAR, hs::kPackLidarW, 0) && pack_table(HS_EXPORT_AGENT_OBS, hs::kPackAgentN, hs::kPackAgentW) &&
              pack_table(HS_EXPORT_BOX_OBS, hs::kPackBoxN, hs::kPackBoxW) && pack_table(HS_EXPORT_RAMP_OBS, hs::kPackRampN, hs::kPackRampW) &&
              pack_table(HS_EXPORT_AGENT_VIS_MASKS, hs::kPackAgentN, 1) && pack_table(HS_EXPORT_BOX_VIS_MASKS, hs::kPackBoxN, 1) &&
              pack_table(HS_EXPORT_RAMP_VIS_MASKS, hs::kPackRampN, 1), "k_pack's widths are those of kExports");
static_assert(HS_PACK_ROW == hs::kPackRow && HS_PACK_MOMENTS == hs::kPackMoments, "hs_pack_request layout");

size_t bytes_of(const hs_sim *s, int id) {
    const hs_tensor_desc &d = s->exports[id];
    return (size_t)(d.dims[0] * d.dims[1] * d.dims[2] * d.dims[3]) * (d.dtype == HS_DTYPE_U8 ? 1 : 4);
}
// Describe export `id` and allocate it, zero-filled: a dim of 0 is absent, the rest of dims[] is padded with 1.
int alloc_export(hs_sim *s, int id, int dtype, std::initializer_list<int64_t> dims) {
    hs_tensor_desc &d = s->exports[id];
    d.dtype = dtype; d.ndim = 0; d.gpu_id = s->cfg.gpu_id;
    for (int64_t v : dims) if (v) d.dims[d.ndim++] = v;
    for (int i = d.ndim; i < 4; ++i) d.dims[i] = 1;
    uint8_t *p;
    HS_TRY(s->dalloc(&p, bytes_of(s, id)));
    d.ptr = p;
    return HS_OK;
}

// The renderer outputs (Manager::depthTensor / rgbTensor, src/mgr.cpp:1241-1263): allocated on first need, zero-filled.
int ensure_render_buffers(hs_sim *s) {
    const int64_t r = (int64_t)s->S.N * s->A;
    const int64_t H = s->cfg.batch_render_height > 0 ? s->cfg.batch_render_height : 64;
    const int64_t Wd = s->cfg.batch_render_width > 0 ? s->cfg.batch_render_width : 64;
    if (!s->exports[HS_EXPORT_RGB].ptr) HS_TRY(alloc_export(s, HS_EXPORT_RGB, HS_DTYPE_U8, {r, H, Wd, 4}));
    if (!s->exports[HS_EXPORT_DEPTH].ptr) HS_TRY(alloc_export(s, HS_EXPORT_DEPTH, HS_DTYPE_F32, {r, H, Wd, 1}));
    return HS_OK;
}
// k_render over every view (hs_k_render.h); the buffers exist (ensure_render_buffers).
void launch_render(hs_sim *s, hipStream_t strm) {
    const hs_tensor_desc &d = s->exports[HS_EXPORT_DEPTH];
    const int nslots = (s->S.N + hs::kTile - 1) / hs::kTile * hs::kTile;
    hipLaunchKernelGGL(hs::k_render, dim3(nslots * s->A), dim3(hs::kRenderThreads), 0, strm, s->S, (float *)d.ptr,
                       (unsigned *)s->exports[HS_EXPORT_RGB].ptr, (int)d.dims[2], (int)d.dims[1]);
}

// (serve / step_idx: the group of octets the launch observes and the ring position of the step's groups, hs_state.h)
void launch_observe(hs_sim *s, hipStream_t strm, int serve = hs::kGroupAll, int step_idx = 0) {
    hs::SimState S = s->S;
    if (S.flags & hs::FLAG_EXT_SKIP_OBSERVATIONS) return;
    S.stepIdx = hs::step_idx_arg(step_idx, serve);
    struct RenderAfter {        // HS_FLAG_EXT_RENDER: the agent views are part of every step's observations
        hs_sim *s; hipStream_t strm;
        ~RenderAfter() { if ((s->S.flags & hs::FLAG_EXT_RENDER) && s->exports[HS_EXPORT_DEPTH].ptr) launch_render(s, strm); }
    } render_after{s, strm};
    // one workgroup per world; the grid covers whole groups of 8 octets (k_observe's block -> world mapping)
    const int N = ((S.N + hs::kTile - 1) / hs::kTile + 7) / 8 * 64;
    const int nt = hs::obs_threads(s->A);                          // a lane per ray (hs_k_observe.h)
    if (nt <= 128) hipLaunchKernelGGL(hs::k_observe<128>, dim3(N), dim3(128), 0, strm, S);
    else if (nt <= 192) hipLaunchKernelGGL(hs::k_observe<192>, dim3(N), dim3(192), 0, strm, S);
    else hipLaunchKernelGGL(hs::k_observe<320>, dim3(N), dim3(320), 0, strm, S);
}

// Deal the worlds to the octets by contact load (hs_k_balance.h), every kBalancePeriod steps: histogram, scan, deal, one copy
// of the column arena, one move kernel over all columns, commit (six launches and a copy; it was 26 launches and 11 copies).
int order_after_default_stream(hs_sim *s);

int balance_worlds(hs_sim *s, hipStream_t strm) {
    const hs::SimState &S = s->S;
    const int nfull = S.N / hs::kTile * hs::kTile;
    if (nfull < 2 * hs::kTile) return HS_OK;
    const dim3 grid((nfull + 255) / 256), blk(256);
    hipLaunchKernelGGL(hs::k_balance_hist, grid, blk, 0, strm, S, nfull, s->bal_hist);
    hipLaunchKernelGGL(hs::k_balance_scan, dim3(1), dim3(hs::kBalanceBins), 0, strm, s->bal_hist, s->bal_cursor);
    hipLaunchKernelGGL(hs::k_balance_deal, grid, blk, 0, strm, S, nfull, s->bal_cursor, s->bal_new_slot);
    HS_HIP(hipMemcpyAsync(s->bal_tmp, s->col_arena, s->col_arena_bytes, hipMemcpyDeviceToDevice, strm));
    const size_t n = (size_t)nfull * s->bal_cols.base[hs::kBalanceCols];
    hipLaunchKernelGGL(hs::k_balance_move_all, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, strm, (int *)s->col_arena, (const int *)s->bal_tmp,
                       s->bal_cols, s->col_slots, (const int *)s->S.slotOfWorld, (const int *)s->bal_new_slot, nfull);
    hipLaunchKernelGGL(hs::k_balance_commit, grid, blk, 0, strm, S, nfull, (const int *)s->bal_new_slot);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

void launch_physics(hs_sim *s, hipStream_t strm, const hs::SimState &S) {
    const int noct = (S.N + hs::kTile - 1) / hs::kTile;
    // rounds of 64 lanes over the octet's bodies: 16 body slots per world with up to 5 agents, 17 with 6
    if (s->A > hs::kMaxAgents - 1) hipLaunchKernelGGL(hs::k_physics<3>, dim3(noct), dim3(hs::kPhysThreads), 0, strm, S);
    else hipLaunchKernelGGL(hs::k_physics<2>, dim3(noct), dim3(hs::kPhysThreads), 0, strm, S);
}

// One step = k_physics (movement + actionSystem, 4 XPBD substeps, rewards / dones / episode results, reset: one
// kernel, a wave per octet of 8 worlds, hs_k_physics.h) and k_observe.  Manager::init = k_reset then k_observe.
//
// `split` (the blocking hs_step only, whose caller waits for the whole device anyway): the step runs as two independent
// chains, k_physics -> k_observe of the late octets on `strm` and k_physics -> k_observe of the early octets on the
// handle's own stream, ordered after what `strm` (the legacy default stream) held before the step.  Worlds never
// interact and every export is indexed by world id, so the chains share nothing but the commuting tick sum; the early
// group's k_observe fills the SIMDs its physics waves have left while the slowest physics waves finish.  The
// dependencies are kernel boundaries only.  The caller waits for both streams (hs_step_end).  The steps that keep the
// one-chain schedule: the one with the periodic deal, profiled steps (ev[0..3] bracket whole kernels), observations
// skipped or followed by k_render.
int launch_step(hs_sim *s, hipStream_t strm, bool first, bool split = false) {
    if (!first && ++s->steps_since_balance >= hs::kBalancePeriod) {
        s->steps_since_balance = 0;
        split = false;
        int rc = balance_worlds(s, strm);
        if (rc != HS_OK) return rc;
    }
    const bool prof = s->profiling;
    hs::SimState S = s->S;
    const int N = S.N;
    const int sidx = s->step_idx;
    S.stepIdx = hs::step_idx_arg(sidx, hs::kGroupAll); if (!first) s->step_idx = (s->step_idx + 1) % 3;
    if (split && s->split_fits && !first && !prof && !(S.flags & (hs::FLAG_EXT_SKIP_OBSERVATIONS | hs::FLAG_EXT_RENDER))) {
        HS_TRY(order_after_default_stream(s));       // (before the late chain is queued on the default stream)
        S.stepIdx = hs::step_idx_arg(sidx, hs::kGroupLate);
        launch_physics(s, strm, S);
        launch_observe(s, strm, hs::kGroupLate, sidx);
        S.stepIdx = hs::step_idx_arg(sidx, hs::kGroupEarly);
        launch_physics(s, s->stream, S);
        launch_observe(s, s->stream, hs::kGroupEarly, sidx);
        s->split_open = true; ++s->split_steps;
        HS_HIP(hipGetLastError());
        return HS_OK;
    }
    if (prof) HS_HIP(hipEventRecord(s->ev[0], strm));
    if (!first) launch_physics(s, strm, S);
    if (prof) HS_HIP(hipEventRecord(s->ev[1], strm));
    // in a step the reset is the tail of k_physics; only Manager::init launches it on its own
    if (first) hipLaunchKernelGGL(hs::k_reset, dim3((N + 31) / 32), dim3(32), 0, strm, S);     // half-filled waves: the generator diverges per world
    if (prof) HS_HIP(hipEventRecord(s->ev[2], strm));
    launch_observe(s, strm);
    if (prof) HS_HIP(hipEventRecord(s->ev[3], strm));
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// A failure of an earlier asynchronous entry point (the XLA custom calls have no status channel) surfaces at the next call
// that can report it.  Nothing here touches the device: the sticky counters of hs_get_device_status (candidate pairs
// that took the spill path) are read only on request, so no step ever pays a blocking copy for them.
int poll_status(hs_sim *s) {
    const int32_t e = s->async_error.exchange(0);
    if (e != 0) return fail(HS_ERR_HIP, "an XLA custom call on this simulator failed earlier with status " + std::to_string(e));
    return HS_OK;
}

}  // namespace

// ==== the learner calls ====
// Each section below has the static_asserts that tie a request of hideseek.h to its kernel header, a check_* that refuses
// a bad request with "<entry point>: <what>", and a launch_* that enqueues the kernels of an accepted one.  The order of
// the sections and of the launches in them is the order in which the compiler instantiates the kernels, and it is kept:
// the compiler numbers functions, and with them the branch labels of the device assembly, in order of emission, so a
// kernel instantiated earlier or later than before would no longer compare equal to itself (tools/isa_diff.py, DESIGN.md
// section 5).  Hence launch_* are ordinary functions, a new stage goes after the last one, and a kernel is launched from a
// template only where that template is instantiated at its call (with_elem, by its deduced return type) or where the
// kernel has always been launched from one (launch_pack_as, launch_pack_moments_sum<>, the with_* of an absent array).
// What the row-wise kernels (k_embed, k_lstm, k_dense) share, and the one fixed-order sum kernel of every stage, is in
// hs_rows.h.
namespace {
// ---- what the checks share ----
size_t elem_size(int32_t dtype) { return dtype == HS_DTYPE_F32 ? 4u : 2u; }
bool dtype_ok(int32_t d) { return d == HS_DTYPE_F32 || d == HS_DTYPE_BF16 || d == HS_DTYPE_F16; }
// every pointer (null included) is a multiple of k, a power of two
bool aligned(uintptr_t k, std::initializer_list<const void *> ps) {
    uintptr_t bits = 0;
    for (const void *p : ps) bits |= (uintptr_t)p;
    return !(bits & (k - 1));
}
// n at least 1 and n * stride below 2^31 for every stride: the kernels index with int
bool count_ok(int32_t n, std::initializer_list<int64_t> strides) {
    for (int64_t st : strides)
        if ((int64_t)n * st >= (int64_t)1 << 31) return false;
    return n >= 1;
}
// The bytes an argument covers; a null argument covers none.
struct ByteRange { const char *name; uintptr_t lo, hi; };
ByteRange range(const char *name, const void *p, uintptr_t bytes) { return {name, (uintptr_t)p, p ? (uintptr_t)p + bytes : 0}; }
bool overlap(const ByteRange &a, const ByteRange &b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

// The entry point a check speaks for: its failures read "<fn>: <what>", and the string is built only then.
struct Check {
    const char *fn;
    int bad(const std::string &what, int code = HS_ERR_INVALID_ARG) const { return fail(code, std::string(fn) + ": " + what); }
    int dtype(int32_t d, const char *what) const {
        return dtype_ok(d) ? HS_OK : bad(std::string(what) + " dtype must be HS_DTYPE_F32, HS_DTYPE_BF16 or HS_DTYPE_F16");
    }
    // no output overlaps an input or an earlier output
    int disjoint(const ByteRange *in, size_t nin, const ByteRange *out, size_t nout) const {
        for (const ByteRange *o = out; o != out + nout; ++o) {
            for (const ByteRange *x = in; x != in + nin; ++x)
                if (overlap(*o, *x)) return bad(std::string(o->name) + " overlaps " + x->name);
            for (const ByteRange *e = out; e != o; ++e)
                if (overlap(*o, *e)) return bad(std::string(o->name) + " overlaps " + e->name);
        }
        return HS_OK;
    }
    int disjoint(std::initializer_list<ByteRange> in, std::initializer_list<ByteRange> out) const {
        return disjoint(in.begin(), in.size(), out.begin(), out.size());
    }
    // the same over a request's ranges as one list, the first `nin` of them its inputs
    int disjoint(const std::vector<ByteRange> &v, size_t nin) const { return disjoint(v.data(), nin, v.data() + nin, v.size() - nin); }
    // `x`, a trailing argument, overlaps none of them
    int apart(const ByteRange &x, const std::vector<ByteRange> &v) const {
        for (const ByteRange &y : v)
            if (overlap(x, y)) return bad(std::string(x.name) + " overlaps " + y.name);
        return HS_OK;
    }
    // the learner calls read what a finished hs_init / step left
    int handle_ready(const hs_sim *s) const {
        if (!s->initialised) return fail(HS_ERR_INVALID_ARG, std::string(fn) + " before hs_init");
        if (s->step_open) return fail(HS_ERR_INVALID_ARG, std::string(fn) + " inside an open step");
        return HS_OK;
    }
    // the heads' bucket counts of a multi-discrete actor (sampler and PPO loss); *L is their sum
    int buckets(const int32_t *k, int *L) const {
        *L = 0;
        for (int h = 0; h < HS_SAMPLE_HEADS; ++h) {
            if (k[h] < 1 || k[h] > HS_SAMPLE_MAX_BUCKETS) return bad("a bucket count must be in [1, HS_SAMPLE_MAX_BUCKETS]");
            *L += k[h];
        }
        return *L > HS_SAMPLE_MAX_LOGITS ? bad("more than HS_SAMPLE_MAX_LOGITS logits per row") : HS_OK;
    }
};
// the bucket counts that passed Check::buckets as the kernels take them, a byte per head: the count and the first logit;
// returns their sum
int pack_buckets(const int32_t *k, uint64_t *bucketK, uint64_t *bucketOff) {
    int off = 0;
    for (int h = 0; h < HS_SAMPLE_HEADS; off += k[h++]) {
        *bucketK |= (uint64_t)k[h] << (8 * h);
        *bucketOff |= (uint64_t)off << (8 * h);
    }
    return off;
}

// ---- what the launches share ----
// f(tag) with tag's type the element type of an array of type `dtype`.  The return type is deduced so that a call
// instantiates f's body, and the kernels it launches, at that place in the file.
template <typename F> auto with_elem(int32_t dtype, F f) {
    if (dtype == HS_DTYPE_F32) f(float{});
    else if (dtype == HS_DTYPE_BF16) f(hs::SampleBf16{});
    else f(hs::SampleF16{});
}
// the same for an array that may be absent (null)
template <typename F> void with_optional_elem(const void *p, int32_t dtype, F f) {
    if (!p) f(hs::PpoAbsent{});
    else with_elem(dtype, f);
}
// f(std::integral_constant<int, V>) for the V of Vs that `v` is.  A left fold: the compiler instantiates f for the Vs in
// the order written (a right fold goes from the last to the first).
template <int... Vs, typename F> void with_constant(int32_t v, F f) {
    (void)(... || (v == Vs && (f(std::integral_constant<int, Vs>{}), true)));
}
// the element type of an array as the row-wise kernels take it, a run-time code
int elem_code(int32_t dtype) { return dtype == HS_DTYPE_F32 ? hs::kElemF32 : dtype == HS_DTYPE_BF16 ? hs::kElemBf16 : hs::kElemF16; }
// The fixed-order sum of a stage's `nparts` workspace slices of `len` values into `out`.  The return type is deduced, as
// with_elem's, so that a call instantiates k_partials_sum at that place in the file.
template <typename T, int kCols, int kSegs> auto launch_partials_sum(hipStream_t strm, const T *partials, int nparts, int len, T *out) {
    hipLaunchKernelGGL((hs::k_partials_sum<T, kCols, kSegs>), dim3((len + kCols - 1) / kCols), dim3(kCols * kSegs), 0, strm, partials, nparts, len, out);
}
}  // namespace

// ---- policy inputs (hs_k_pack.h) ----
namespace {
template <typename TA, typename TC, bool MOM> void launch_pack_as(const hs::PackArgs &a, hipStream_t strm) {
    if constexpr (std::is_same<TA, hs::PackAbsent>::value && std::is_same<TC, hs::PackAbsent>::value && !MOM) return;
    else hipLaunchKernelGGL((hs::k_pack<TA, TC, MOM>), dim3(hs::pack_grid(a.rows)), dim3(hs::kPackThreads), 0, strm, a);
}
// f(tag) with the element type of output `p` of type `dtype` as tag's type: k_pack has tags of its own
template <typename F> void with_pack_type(const void *p, int32_t dtype, F f) {
    if (!p) f(hs::PackAbsent{});
    else if (dtype == HS_DTYPE_F32) f(float{});
    else if (dtype == HS_DTYPE_BF16) f(hs::PackBf16{});
    else f(hs::PackF16{});
}

// The one check that looks at the handle before the arguments.
int check_pack(hs_sim *s, const hs_pack_request *r) {
    const Check c{"hs_pack_policy_inputs"};
    if (!r) return c.bad("null request");
    if (s->S.flags & hs::FLAG_EXT_SKIP_OBSERVATIONS) return c.bad("HS_FLAG_EXT_SKIP_OBSERVATIONS leaves no observations to pack", HS_ERR_UNSUPPORTED);
    HS_TRY(c.handle_ready(s));
    if (!r->actor && !r->critic && !r->moments) return c.bad("every output is null");
    if (r->actor) HS_TRY(c.dtype(r->actor_dtype, "output"));
    if (r->critic) HS_TRY(c.dtype(r->critic_dtype, "output"));
    if (!aligned(16, {r->actor, r->critic})) return c.bad("outputs must be 16-byte aligned");
    if (!aligned(8, {r->moments})) return c.bad("moments must be 8-byte aligned");
    return HS_OK;
}
// The fixed-order sum of the workgroups' moments, after a k_pack or k_pack_norm that wrote them.  A template, so that
// its k_partials_sum is instantiated after the k_pack kernels of launch_pack.
template <int kSegs = hs::kPackSumSegs>
int launch_pack_moments_sum(hs_sim *s, hipStream_t strm, const hs_pack_request *r, int rows) {
    if (r->moments) launch_partials_sum<double, hs::kPackThreads / kSegs, kSegs>(strm, s->pack_partials, hs::pack_grid(rows), hs::kPackMoments, r->moments);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
hs::PackArgs pack_args(hs_sim *s, const hs_pack_request *r) {
    const hs::SimState &S = s->S;
    return {S.xPrep, S.xSelfType, S.xSelfObs, S.xSelfMask, S.xLidar, S.xAgentObs, S.xBoxObs, S.xRampObs,
            S.xVisAgents, S.xVisBoxes, S.xVisRamps, r->actor, r->critic, s->pack_partials, S.N * s->A};
}
// One k_pack over every agent row (the request has passed check_pack), then the fixed-order sum of the moments.
int launch_pack(hs_sim *s, hipStream_t strm, const hs_pack_request *r) {
    const hs::PackArgs a = pack_args(s, r);
    with_pack_type(r->actor, r->actor_dtype, [&](auto ta) {
        with_pack_type(r->critic, r->critic_dtype, [&](auto tc) {
            if (r->moments) launch_pack_as<decltype(ta), decltype(tc), true>(a, strm);
            else launch_pack_as<decltype(ta), decltype(tc), false>(a, strm);
        });
    });
    return launch_pack_moments_sum<>(s, strm, r, a.rows);
}
}  // namespace

// ---- action sampling (hs_k_sample.h) ----
namespace {
static_assert(HS_SAMPLE_HEADS == hs::kSampleHeads && HS_SAMPLE_MAX_BUCKETS == hs::kSampleMaxBuckets && HS_SAMPLE_MAX_LOGITS == hs::kSampleMaxLogits &&
              HS_SAMPLE_DRAW == hs::kSampleDraw && HS_SAMPLE_GREEDY == hs::kSampleGreedy && HS_SAMPLE_EVALUATE == hs::kSampleEvaluate,
              "hs_sample_request and k_sample agree");
static_assert(kExports[HS_EXPORT_ACTION].tail[0] == HS_SAMPLE_HEADS && kExports[HS_EXPORT_ACTION].dtype == HS_DTYPE_I32, "k_sample writes the action export's rows");

int check_sample(hs_sim *s, const hs_sample_request *r) {
    const Check c{"hs_sample_actions"};
    if (!r) return c.bad("null request");
    if (!r->logits) return c.bad("null logits");
    HS_TRY(c.dtype(r->logits_dtype, "logits"));
    if (r->mode != HS_SAMPLE_DRAW && r->mode != HS_SAMPLE_GREEDY && r->mode != HS_SAMPLE_EVALUATE) return c.bad("unknown mode");
    if (r->flags & ~(uint32_t)HS_SAMPLE_ZERO_INACTIVE) return c.bad("unknown flag");
    int L;
    HS_TRY(c.buckets(r->buckets, &L));
    if (r->logits_stride < L) return c.bad("logits_stride is below the sum of the buckets");
    if (!aligned(elem_size(r->logits_dtype), {r->logits})) return c.bad("logits must be aligned to their element size");
    if (!aligned(4, {r->action, r->log_prob, r->entropy, r->head_log_prob})) return c.bad("action, log_prob, entropy and head_log_prob must be 4-byte aligned");
    if (r->mode == HS_SAMPLE_EVALUATE && !r->log_prob && !r->entropy && !r->head_log_prob) return c.bad("HS_SAMPLE_EVALUATE with every output null");
    HS_TRY(c.handle_ready(s));
    if ((r->flags & HS_SAMPLE_ZERO_INACTIVE) && (s->S.flags & hs::FLAG_EXT_SKIP_OBSERVATIONS))
        return c.bad("HS_SAMPLE_ZERO_INACTIVE needs self_mask, which HS_FLAG_EXT_SKIP_OBSERVATIONS leaves unwritten", HS_ERR_UNSUPPORTED);
    return HS_OK;
}
// One k_sample over every agent row (the request has passed check_sample).
int launch_sample(hs_sim *s, hipStream_t strm, const hs_sample_request *r) {
    const hs::SimState &S = s->S;
    hs::SampleArgs a = {};
    a.logits = r->logits;
    a.actionIn = a.action = r->action ? r->action : S.xAction;
    a.selfMask = (r->flags & HS_SAMPLE_ZERO_INACTIVE) ? S.xSelfMask : nullptr;
    a.logProb = r->log_prob; a.entropy = r->entropy; a.headLogProb = r->head_log_prob;
    a.L = pack_buckets(r->buckets, &a.bucketK, &a.bucketOff);
    a.rows = S.N * s->A; a.stride = r->logits_stride; a.mode = r->mode;
    a.seed0 = r->seed[0]; a.seed1 = r->seed[1]; a.counter = r->counter;
    a.row0Global = (uint32_t)S.worldOffset * (uint32_t)s->A;
    const dim3 grid(hs::sample_grid(a.rows)), blk(hs::kSampleThreads);
    with_elem(r->logits_dtype, [&](auto t) { hipLaunchKernelGGL(hs::k_sample<decltype(t)>, grid, blk, 0, strm, a); });
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- advantages and value targets (hs_k_gae.h) ----
namespace {
static_assert(HS_GAE_MAX_STEPS == hs::kGaeMaxSteps && HS_GAE_MOMENTS == hs::kGaeMoments, "hs_gae_request and k_gae agree");
static_assert(sizeof(hs_gae_request) == 80 && offsetof(hs_gae_request, value_dtype) == 40 && offsetof(hs_gae_request, gamma) == 48 &&
              offsetof(hs_gae_request, advantage) == 56 && offsetof(hs_gae_request, moments) == 72, "hs_gae_request layout (gpu_hideseek/advantages.py mirrors it)");
static_assert(kExports[HS_EXPORT_REWARD].dtype == HS_DTYPE_F32 && kExports[HS_EXPORT_DONE].dtype == HS_DTYPE_I32 && kExports[HS_EXPORT_SELF_MASK].dtype == HS_DTYPE_F32 &&
              kExports[HS_EXPORT_REWARD].per_agent && kExports[HS_EXPORT_DONE].per_agent && kExports[HS_EXPORT_SELF_MASK].per_agent,
              "k_gae reads copies of the reward, done and self_mask exports");

// What hs_compute_gae and hs_compute_gae_grouped check of a request: `groups` moments vectors.
int check_gae_request(const Check &c, hs_sim *s, const hs_gae_request *r, int groups) {
    if (!r->reward) return c.bad("null reward");
    if (!r->done) return c.bad("null done");
    if (!r->value) return c.bad("null value");
    if (!r->bootstrap) return c.bad("null bootstrap");
    if (!r->advantage && !r->returns && !r->moments) return c.bad("every output is null");
    HS_TRY(c.dtype(r->value_dtype, "value"));
    if (r->steps < 1 || r->steps > HS_GAE_MAX_STEPS) return c.bad("steps must be in [1, HS_GAE_MAX_STEPS]");
    if (!(r->gamma >= 0.f && r->gamma <= 1.f)) return c.bad("gamma must be finite and in [0, 1]");
    if (!(r->lambda >= 0.f && r->lambda <= 1.f)) return c.bad("lambda must be finite and in [0, 1]");
    const uintptr_t vsize = elem_size(r->value_dtype);
    if (!aligned(4, {r->reward, r->done, r->mask, r->advantage, r->returns})) return c.bad("reward, done, mask, advantage and returns must be 4-byte aligned");
    if (!aligned(vsize, {r->value, r->bootstrap})) return c.bad("value and bootstrap must be aligned to their element size");
    if (!aligned(8, {r->moments})) return c.bad("moments must be 8-byte aligned");
    const uintptr_t rows = (uintptr_t)s->S.N * (uintptr_t)s->A, n = rows * (uintptr_t)r->steps;
    HS_TRY(c.disjoint({range("reward", r->reward, n * 4), range("done", r->done, n * 4), range("value", r->value, n * vsize),
                       range("bootstrap", r->bootstrap, rows * vsize), range("mask", r->mask, n * 4)},
                      {range("advantage", r->advantage, n * 4), range("returns", r->returns, n * 4),
                       range("moments", r->moments, (uintptr_t)groups * HS_GAE_MOMENTS * sizeof(double))}));
    return c.handle_ready(s);
}
int check_gae(hs_sim *s, const hs_gae_request *r) {
    const Check c{"hs_compute_gae"};
    if (!r) return c.bad("null request");
    return check_gae_request(c, s, r, 1);
}
// One k_gae over every agent row (the request has passed check_gae), then the fixed-order sum of the moments.
int launch_gae(hs_sim *s, hipStream_t strm, const hs_gae_request *r) {
    const hs::GaeArgs a = {r->reward, r->done, r->value, r->bootstrap, r->mask, r->advantage, r->returns,
                           r->moments ? s->gae_partials : nullptr, s->S.N * s->A, r->steps, r->gamma, r->lambda};
    const dim3 grid(hs::gae_grid(a.rows)), blk(hs::kGaeThreads);
    with_elem(r->value_dtype, [&](auto t) { hipLaunchKernelGGL(hs::k_gae<decltype(t)>, grid, blk, 0, strm, a); });
    if (r->moments) launch_partials_sum<double, hs::kGaeMoments, hs::kGaeSumSegs>(strm, s->gae_partials, hs::gae_grid(a.rows), hs::kGaeMoments, r->moments);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the PPO loss and its gradients (hs_k_ppo.h) ----
namespace {
static_assert(HS_PPO_STATS == hs::kPpoStats && HS_GAE_MOMENTS == hs::kGaeMoments, "hs_ppo_request and k_ppo agree");
static_assert(sizeof(hs_ppo_request) == 160 && offsetof(hs_ppo_request, n) == 72 && offsetof(hs_ppo_request, buckets) == 96 &&
              offsetof(hs_ppo_request, clip_coef) == 116 && offsetof(hs_ppo_request, grad_logits) == 136 && offsetof(hs_ppo_request, stats) == 152,
              "hs_ppo_request layout (gpu_hideseek/ppo_loss.py mirrors it)");

// The bytes a request whose counts, strides and dtypes have passed reads (the first *nin ranges) and writes.
std::vector<ByteRange> ppo_ranges(const hs_ppo_request *r, int L, size_t *nin) {
    const uintptr_t lsize = elem_size(r->logits_dtype), gsize = elem_size(r->grad_dtype), vsize = elem_size(r->value_dtype), n = (uintptr_t)r->n;
    *nin = 9;
    return {range("logits", r->logits, ((n - 1) * (uintptr_t)r->logits_stride + L) * lsize), range("action", r->action, n * HS_SAMPLE_HEADS * 4),
            range("old_log_prob", r->old_log_prob, n * 4), range("advantage", r->advantage, n * 4),
            range("adv_moments", r->adv_moments, HS_GAE_MOMENTS * sizeof(double)), range("mask", r->mask, n * 4),
            range("value", r->value, n * vsize), range("returns", r->returns, n * 4), range("old_value", r->old_value, n * 4),
            range("grad_logits", r->grad_logits, ((n - 1) * (uintptr_t)r->grad_stride + L) * gsize),
            range("grad_value", r->grad_value, n * vsize), range("stats", r->stats, HS_PPO_STATS * sizeof(double))};
}

int check_ppo(hs_sim *s, const hs_ppo_request *r) {
    const Check c{"hs_ppo_loss"};
    if (!r) return c.bad("null request");
    if (!r->logits) return c.bad("null logits");
    if (!r->action) return c.bad("null action");
    if (!r->old_log_prob) return c.bad("null old_log_prob");
    if (!r->advantage) return c.bad("null advantage");
    if (!r->grad_logits && !r->grad_value && !r->stats) return c.bad("every output is null");
    if (r->grad_value && !r->value) return c.bad("grad_value without value");
    if (r->value && !r->returns) return c.bad("value without returns");
    if (!r->value && (r->returns || r->old_value)) return c.bad("returns or old_value without value");
    HS_TRY(c.dtype(r->logits_dtype, "logits"));
    if (r->grad_logits) HS_TRY(c.dtype(r->grad_dtype, "grad"));
    if (r->value) HS_TRY(c.dtype(r->value_dtype, "value"));
    int L;
    HS_TRY(c.buckets(r->buckets, &L));
    if (r->logits_stride < L) return c.bad("logits_stride is below the sum of the buckets");
    if (r->grad_logits && r->grad_stride < L) return c.bad("grad_stride is below the sum of the buckets");
    if (!count_ok(r->n, {r->logits_stride, r->grad_logits ? r->grad_stride : 0})) return c.bad("n must be at least 1 and n * stride below 2^31");
    if (!std::isfinite(r->clip_coef) || !(r->clip_coef > 0.f)) return c.bad("clip_coef must be finite and above 0");
    if (!std::isfinite(r->value_loss_coef) || !std::isfinite(r->entropy_coef) || !std::isfinite(r->grad_scale))
        return c.bad("value_loss_coef, entropy_coef and grad_scale must be finite");
    const uintptr_t lsize = elem_size(r->logits_dtype), gsize = elem_size(r->grad_dtype), vsize = elem_size(r->value_dtype);
    if (!aligned(4, {r->action, r->old_log_prob, r->advantage, r->mask, r->returns, r->old_value}))
        return c.bad("action, old_log_prob, advantage, mask, returns and old_value must be 4-byte aligned");
    if (!aligned(lsize, {r->logits}) || !aligned(gsize, {r->grad_logits}) || !aligned(vsize, {r->value, r->grad_value}))
        return c.bad("logits, grad_logits, value and grad_value must be aligned to their element size");
    if (!aligned(8, {r->adv_moments, r->stats})) return c.bad("adv_moments and stats must be 8-byte aligned");
    size_t nin;
    const std::vector<ByteRange> v = ppo_ranges(r, L, &nin);
    HS_TRY(c.disjoint(v, nin));
    return c.handle_ready(s);
}

// With a mask the count of the active samples, then one k_ppo over the samples (the request has passed check_ppo), then
// the fixed-order sum of the statistics.
hs::PpoArgs ppo_args(hs_sim *s, const hs_ppo_request *r) {
    hs::PpoArgs a = {};
    a.logits = r->logits; a.action = r->action; a.oldLogProb = r->old_log_prob; a.advantage = r->advantage;
    a.advMoments = r->adv_moments; a.mask = r->mask; a.value = r->value; a.returns = r->returns; a.oldValue = r->old_value;
    a.gradLogits = r->grad_logits; a.gradValue = r->grad_value; a.partials = r->stats ? s->ppo_partials : nullptr;
    a.counts = s->ppo_counts;
    a.L = pack_buckets(r->buckets, &a.bucketK, &a.bucketOff);
    a.n = r->n; a.stride = r->logits_stride; a.gradStride = r->grad_stride; a.countParts = hs::ppo_count_grid(a.n);
    a.clip = r->clip_coef; a.valueCoef = r->value_loss_coef; a.entropyCoef = r->entropy_coef; a.gradScale = r->grad_scale;
    return a;
}
int launch_ppo(hs_sim *s, hipStream_t strm, const hs_ppo_request *r) {
    const hs::PpoArgs a = ppo_args(s, r);
    const dim3 grid(hs::ppo_grid(a.n)), blk(hs::kPpoThreads);
    if (r->mask) hipLaunchKernelGGL(hs::k_ppo_count<>, dim3(a.countParts), blk, 0, strm, r->mask, a.n, s->ppo_counts);
    with_elem(r->logits_dtype, [&](auto tl) {
        with_optional_elem(r->grad_logits, r->grad_dtype, [&](auto tg) {
            with_optional_elem(r->value, r->value_dtype, [&](auto tv) {
                hipLaunchKernelGGL((hs::k_ppo<decltype(tl), decltype(tg), decltype(tv)>), grid, blk, 0, strm, a);
            });
        });
    });
    if (r->stats) launch_partials_sum<double, hs::kPpoStats, hs::kPpoSumSegs>(strm, s->ppo_partials, hs::ppo_grid(a.n), hs::kPpoStats, r->stats);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- observation normaliser (hs_k_norm.h) ----
namespace {
static_assert(HS_NORM_STATE == hs::kNormState && HS_NORM_TABLE == hs::kNormTable && HS_NORM_MAX_MOMENTS == hs::kNormMaxMoments &&
              HS_NORM_STATE == HS_PACK_MOMENTS, "hs_obs_norm_request and k_norm_update agree");
static_assert(hs::norm_skipped(HS_NORM_SKIP_PREP_COUNTER) && hs::norm_skipped(HS_NORM_SKIP_SELF_TYPE) && HS_NORM_SKIP_SELF_TYPE == hs::kPackColType,
              "the skipped columns are prep_counter and self_type");
static_assert(sizeof(hs_obs_norm_request) == 48 && offsetof(hs_obs_norm_request, num_moments) == 8 && offsetof(hs_obs_norm_request, decay) == 16 &&
              offsetof(hs_obs_norm_request, eps) == 24 && offsetof(hs_obs_norm_request, state) == 32 && offsetof(hs_obs_norm_request, table) == 40,
              "hs_obs_norm_request layout (gpu_hideseek/policy_inputs.py mirrors it)");

int check_norm_update(hs_sim *s, const hs_obs_norm_request *r) {
    const Check c{"hs_obs_norm_update"};
    if (!r) return c.bad("null request");
    if (!r->moments) return c.bad("null moments");
    if (!r->state) return c.bad("null state");
    if (!r->table) return c.bad("null table");
    if (r->num_moments < 1 || r->num_moments > HS_NORM_MAX_MOMENTS) return c.bad("num_moments must be in [1, HS_NORM_MAX_MOMENTS]");
    if (!(r->decay >= 0.0 && r->decay < 1.0)) return c.bad("decay must be in [0, 1)");
    if (!std::isfinite(r->eps) || !(r->eps > 0.0)) return c.bad("eps must be finite and above 0");
    if (!aligned(8, {r->moments, r->state})) return c.bad("moments and state must be 8-byte aligned");
    if (!aligned(16, {r->table})) return c.bad("table must be 16-byte aligned");
    HS_TRY(c.disjoint({range("moments", r->moments, (uintptr_t)r->num_moments * HS_PACK_MOMENTS * sizeof(double))},
                      {range("state", r->state, HS_NORM_STATE * sizeof(double)), range("table", r->table, HS_NORM_TABLE * sizeof(float))}));
    return c.handle_ready(s);
}
int launch_norm_update(hs_sim *, hipStream_t strm, const hs_obs_norm_request *r) {
    const hs::NormArgs a = {r->moments, r->num_moments, r->decay, r->eps, r->state, r->table};
    hipLaunchKernelGGL(hs::k_norm_update<>, dim3(1), dim3(hs::kNormThreads), 0, strm, a);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

int check_pack_norm(hs_sim *s, const hs_pack_request *r, const float *table) {
    const Check c{"hs_pack_policy_inputs_normalized"};
    HS_TRY(check_pack(s, r));
    if (!table) return c.bad("null table");
    if (!aligned(16, {table})) return c.bad("table must be 16-byte aligned");
    return HS_OK;
}
// One k_pack_norm over every agent row (the request has passed check_pack_norm), then the fixed-order sum of the moments.
// With no rows requested the moments alone are those of hs_pack_policy_inputs: the table is not read.
int launch_pack_norm(hs_sim *s, hipStream_t strm, const hs_pack_request *r, const float *table) {
    if (!r->actor && !r->critic) return launch_pack(s, strm, r);
    const hs::PackArgs a = pack_args(s, r);
    const dim3 grid(hs::pack_grid(a.rows)), blk(hs::kPackThreads);
    with_pack_type(r->actor, r->actor_dtype, [&](auto ta) {
        with_pack_type(r->critic, r->critic_dtype, [&](auto tc) {
            if constexpr (std::is_same<decltype(ta), hs::PackAbsent>::value && std::is_same<decltype(tc), hs::PackAbsent>::value) return;
            else if (r->moments) hipLaunchKernelGGL((hs::k_pack_norm<decltype(ta), decltype(tc), true>), grid, blk, 0, strm, a, table);
            else hipLaunchKernelGGL((hs::k_pack_norm<decltype(ta), decltype(tc), false>), grid, blk, 0, strm, a, table);
        });
    });
    return launch_pack_moments_sum<>(s, strm, r, a.rows);
}
}  // namespace

// ---- the two-hot symlog critic head (hs_k_twohot.h) ----
namespace {
static_assert(HS_TWOHOT_STATS == hs::kTwStats && HS_TWOHOT_MAX_BINS == hs::kTwMaxBins, "hs_twohot_request and k_twohot agree");
static_assert(sizeof(hs_twohot_request) == 96 && offsetof(hs_twohot_request, n) == 24 && offsetof(hs_twohot_request, bins) == 36 &&
              offsetof(hs_twohot_request, lo) == 40 && offsetof(hs_twohot_request, value_dtype) == 56 && offsetof(hs_twohot_request, value) == 72 &&
              offsetof(hs_twohot_request, stats) == 88, "hs_twohot_request layout (gpu_hideseek/value_head.py mirrors it)");

// The bytes a request whose counts, strides and dtypes have passed reads (the first *nin ranges) and writes.
std::vector<ByteRange> twohot_ranges(const hs_twohot_request *r, size_t *nin) {
    const uintptr_t lsize = elem_size(r->logits_dtype), gsize = elem_size(r->grad_dtype), vsize = elem_size(r->value_dtype);
    const uintptr_t n = (uintptr_t)r->n, B = (uintptr_t)r->bins;
    *nin = 3;
    return {range("logits", r->logits, ((n - 1) * (uintptr_t)r->logits_stride + B) * lsize), range("returns", r->returns, n * 4),
            range("mask", r->mask, n * 4),
            range("value", r->value, n * vsize), range("grad_logits", r->grad_logits, ((n - 1) * (uintptr_t)r->grad_stride + B) * gsize),
            range("stats", r->stats, HS_TWOHOT_STATS * sizeof(double))};
}

int check_twohot(hs_sim *s, const hs_twohot_request *r) {
    const Check c{"hs_twohot_value"};
    if (!r) return c.bad("null request");
    if (!r->logits) return c.bad("null logits");
    if (!r->value && !r->grad_logits && !r->stats) return c.bad("every output is null");
    if (!r->returns && (r->grad_logits || r->stats)) return c.bad("grad_logits or stats without returns");
    HS_TRY(c.dtype(r->logits_dtype, "logits"));
    if (r->value) HS_TRY(c.dtype(r->value_dtype, "value"));
    if (r->grad_logits) HS_TRY(c.dtype(r->grad_dtype, "grad"));
    if (r->bins < 2 || r->bins > HS_TWOHOT_MAX_BINS) return c.bad("bins must be in [2, HS_TWOHOT_MAX_BINS]");
    const int B = r->bins;
    if (r->logits_stride < B) return c.bad("logits_stride is below bins");
    if (r->grad_logits && r->grad_stride < B) return c.bad("grad_stride is below bins");
    if (!std::isfinite(r->lo) || !std::isfinite(r->hi) || !(r->lo < r->hi)) return c.bad("lo and hi must be finite and lo < hi");
    if (!std::isfinite(r->loss_coef) || !std::isfinite(r->grad_scale)) return c.bad("loss_coef and grad_scale must be finite");
    if (!count_ok(r->n, {r->logits_stride, r->grad_logits ? r->grad_stride : 0})) return c.bad("n must be at least 1 and n * stride below 2^31");
    const uintptr_t lsize = elem_size(r->logits_dtype), gsize = elem_size(r->grad_dtype), vsize = elem_size(r->value_dtype);
    if (!aligned(4, {r->returns, r->mask})) return c.bad("returns and mask must be 4-byte aligned");
    if (!aligned(lsize, {r->logits}) || !aligned(gsize, {r->grad_logits}) || !aligned(vsize, {r->value}))
        return c.bad("logits, grad_logits and value must be aligned to their element size");
    if (!aligned(8, {r->stats})) return c.bad("stats must be 8-byte aligned");
    size_t nin;
    const std::vector<ByteRange> v = twohot_ranges(r, &nin);
    HS_TRY(c.disjoint(v, nin));
    return c.handle_ready(s);
}

// With a mask the count of the active samples, then one k_twohot over the samples (the request has passed
// check_twohot), then the fixed-order sum of the statistics.
hs::TwohotArgs twohot_args(hs_sim *s, const hs_twohot_request *r) {
    hs::TwohotArgs a = {};
    a.logits = r->logits; a.returns = r->returns; a.mask = r->mask; a.value = r->value; a.gradLogits = r->grad_logits;
    a.partials = r->stats ? s->twohot_partials : nullptr; a.counts = s->twohot_counts;
    a.n = r->n; a.stride = r->logits_stride; a.gradStride = r->grad_stride; a.B = r->bins; a.countParts = hs::ppo_count_grid(a.n);
    a.lo = r->lo; a.hi = r->hi; a.lossCoef = r->loss_coef; a.gradScale = r->grad_scale;
    return a;
}
int launch_twohot(hs_sim *s, hipStream_t strm, const hs_twohot_request *r) {
    const hs::TwohotArgs a = twohot_args(s, r);
    const dim3 grid(hs::twohot_grid(a.n)), blk(hs::kTwThreads);
    if (r->mask) hipLaunchKernelGGL(hs::k_ppo_count<>, dim3(a.countParts), dim3(hs::kPpoThreads), 0, strm, r->mask, a.n, s->twohot_counts);
    with_elem(r->logits_dtype, [&](auto tl) {
        with_optional_elem(r->grad_logits, r->grad_dtype, [&](auto tg) {
            with_optional_elem(r->value, r->value_dtype, [&](auto tv) {
                hipLaunchKernelGGL((hs::k_twohot<decltype(tl), decltype(tg), decltype(tv)>), grid, blk, 0, strm, a);
            });
        });
    });
    if (r->stats) launch_partials_sum<double, hs::kTwStats, hs::kTwSumSegs>(strm, s->twohot_partials, hs::twohot_grid(a.n), hs::kTwStats, r->stats);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the entity encoder (hs_k_embed.h) ----
namespace {
static_assert(HS_EMBED_PARAM_ROWS == hs::kEmbParamRows && HS_EMBED_MAX_GRID_BWD == hs::kRowsMaxGridBwd && HS_EMBED_SUM_SEGS == hs::kRowsSumSegs &&
              HS_EMBED_ROWS_PER_WAVE(32) == hs::EmbCfg<32>::kSub && HS_EMBED_ROWS_PER_WAVE(64) == hs::EmbCfg<64>::kSub &&
              HS_EMBED_ROWS_PER_WAVE(128) == hs::EmbCfg<128>::kSub, "hs_entity_encode_request and k_embed agree");
static_assert(sizeof(hs_entity_encode_request) == 56 && offsetof(hs_entity_encode_request, n) == 16 && offsetof(hs_entity_encode_request, embed_dim) == 24 &&
              offsetof(hs_entity_encode_request, eps) == 32 && offsetof(hs_entity_encode_request, features) == 40 &&
              offsetof(hs_entity_encode_request, argmax) == 48, "hs_entity_encode_request layout (gpu_hideseek/entity_encoder.py mirrors it)");
static_assert(sizeof(hs_entity_encode_backward_request) == 64 && offsetof(hs_entity_encode_backward_request, grad_features) == 16 &&
              offsetof(hs_entity_encode_backward_request, argmax) == 24 && offsetof(hs_entity_encode_backward_request, n) == 32 &&
              offsetof(hs_entity_encode_backward_request, grad_dtype) == 44 && offsetof(hs_entity_encode_backward_request, eps) == 48 &&
              offsetof(hs_entity_encode_backward_request, grad_params) == 56, "hs_entity_encode_backward_request layout (gpu_hideseek/entity_encoder.py mirrors it)");

// What the two calls share.
int check_embed_common(const Check &c, const void *rows, const float *params, int32_t n, int32_t rows_dtype, int32_t E, float eps, float slope) {
    if (!rows) return c.bad("null rows");
    if (!params) return c.bad("null params");
    HS_TRY(c.dtype(rows_dtype, "rows"));
    if (E != 32 && E != 64 && E != 128) return c.bad("embed_dim must be 32, 64 or 128");
    if (!count_ok(n, {HS_PACK_ROW, 4 * E})) return c.bad("n must be at least 1 and n * 296 and n * 4 * embed_dim below 2^31");
    if (!std::isfinite(eps) || !std::isfinite(slope) || !(eps > 0.f)) return c.bad("eps and slope must be finite and eps > 0");
    return HS_OK;
}

int check_embed(hs_sim *s, const hs_entity_encode_request *r) {
    const Check c{"hs_entity_encode"};
    if (!r) return c.bad("null request");
    HS_TRY(check_embed_common(c, r->rows, r->params, r->n, r->rows_dtype, r->embed_dim, r->eps, r->slope));
    if (!r->features && !r->argmax) return c.bad("every output is null");
    if (r->features) HS_TRY(c.dtype(r->features_dtype, "features"));
    const uintptr_t rsize = elem_size(r->rows_dtype), fsize = elem_size(r->features_dtype);
    if (!aligned(4, {r->params})) return c.bad("params must be 4-byte aligned");
    if (!aligned(rsize, {r->rows}) || !aligned(fsize, {r->features})) return c.bad("rows and features must be aligned to their element size");
    const uintptr_t n = (uintptr_t)r->n, E = (uintptr_t)r->embed_dim;
    HS_TRY(c.disjoint({range("rows", r->rows, n * HS_PACK_ROW * rsize), range("params", r->params, HS_EMBED_PARAM_ROWS * E * 4)},
                      {range("features", r->features, n * 4 * E * fsize), range("argmax", r->argmax, n * 3 * E)}));
    return c.handle_ready(s);
}

int check_embed_bwd(hs_sim *s, const hs_entity_encode_backward_request *r) {
    const Check c{"hs_entity_encode_backward"};
    if (!r) return c.bad("null request");
    HS_TRY(check_embed_common(c, r->rows, r->params, r->n, r->rows_dtype, r->embed_dim, r->eps, r->slope));
    if (!r->grad_features) return c.bad("null grad_features");
    if (!r->argmax) return c.bad("null argmax");
    if (!r->grad_params) return c.bad("null grad_params");
    HS_TRY(c.dtype(r->grad_dtype, "grad"));
    const uintptr_t rsize = elem_size(r->rows_dtype), gsize = elem_size(r->grad_dtype);
    if (!aligned(4, {r->params, r->grad_params})) return c.bad("params and grad_params must be 4-byte aligned");
    if (!aligned(rsize, {r->rows}) || !aligned(gsize, {r->grad_features})) return c.bad("rows and grad_features must be aligned to their element size");
    const uintptr_t n = (uintptr_t)r->n, E = (uintptr_t)r->embed_dim;
    HS_TRY(c.disjoint({range("rows", r->rows, n * HS_PACK_ROW * rsize), range("params", r->params, HS_EMBED_PARAM_ROWS * E * 4),
                       range("grad_features", r->grad_features, n * 4 * E * gsize), range("argmax", r->argmax, n * 3 * E)},
                      {range("grad_params", r->grad_params, HS_EMBED_PARAM_ROWS * E * 4)}));
    return c.handle_ready(s);
}

// One k_embed_fwd over the rows (the request has passed check_embed).
int launch_embed(hs_sim *, hipStream_t strm, const hs_entity_encode_request *r) {
    hs::EmbedArgs a = {};
    a.rows = r->rows; a.params = r->params; a.features = r->features; a.argmax = r->argmax;
    a.n = r->n; a.rowsType = elem_code(r->rows_dtype); a.featType = elem_code(r->features_dtype); a.eps = r->eps; a.slope = r->slope;
    const dim3 grid(hs::rows_grid(a.n, hs::emb_rows(r->embed_dim), hs::kRowsMaxGrid)), blk(hs::kRowsThreads);
    with_constant<32, 64, 128>(r->embed_dim, [&](auto e) { hipLaunchKernelGGL((hs::k_embed_fwd<decltype(e)::value>), grid, blk, 0, strm, a); });
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// k_embed_bwd into the workspace's slices, then their fixed-order sum (the request has passed check_embed_bwd).
int launch_embed_bwd(hs_sim *s, hipStream_t strm, const hs_entity_encode_backward_request *r) {
    hs::EmbedBwdArgs a = {};
    a.rows = r->rows; a.params = r->params; a.gradFeatures = r->grad_features; a.argmax = r->argmax; a.workspace = s->embed_partials;
    a.n = r->n; a.rowsType = elem_code(r->rows_dtype); a.gradType = elem_code(r->grad_dtype); a.eps = r->eps; a.slope = r->slope;
    const int nparts = hs::rows_grid(a.n, hs::emb_rows(r->embed_dim), hs::kRowsMaxGridBwd), len = hs::kEmbParamRows * r->embed_dim;
    with_constant<32, 64, 128>(r->embed_dim, [&](auto e) { hipLaunchKernelGGL((hs::k_embed_bwd<decltype(e)::value>), dim3(nparts), dim3(hs::kRowsThreads), 0, strm, a); });
    launch_partials_sum<float, hs::kRowsSumCols, hs::kRowsSumSegs>(strm, s->embed_partials, nparts, len, r->grad_params);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the recurrent core (hs_k_lstm.h) ----
namespace {
static_assert(HS_LSTM_PARAM_ROWS == hs::kLstmParamRows && HS_LSTM_MAX_GRID_BWD == hs::kRowsMaxGridBwd && HS_LSTM_MAX_HIDDEN == hs::kLstmMaxH &&
              HS_LSTM_ROWS_PER_ROUND == hs::kRowsWaves, "hs_lstm_cell_request and k_lstm agree");
static_assert(sizeof(hs_lstm_cell_request) == 80 && offsetof(hs_lstm_cell_request, clear) == 24 && offsetof(hs_lstm_cell_request, n) == 32 &&
              offsetof(hs_lstm_cell_request, y_dtype) == 44 && offsetof(hs_lstm_cell_request, eps) == 48 && offsetof(hs_lstm_cell_request, y) == 56 &&
              offsetof(hs_lstm_cell_request, c_next) == 72, "hs_lstm_cell_request layout (gpu_hideseek/recurrent.py mirrors it)");
static_assert(sizeof(hs_lstm_cell_backward_request) == 104 && offsetof(hs_lstm_cell_backward_request, grad_y) == 32 &&
              offsetof(hs_lstm_cell_backward_request, grad_c_next) == 48 && offsetof(hs_lstm_cell_backward_request, n) == 56 &&
              offsetof(hs_lstm_cell_backward_request, y_dtype) == 68 && offsetof(hs_lstm_cell_backward_request, eps) == 72 &&
              offsetof(hs_lstm_cell_backward_request, grad_gates) == 80 && offsetof(hs_lstm_cell_backward_request, grad_cell_params) == 96,
              "hs_lstm_cell_backward_request layout (gpu_hideseek/recurrent.py mirrors it)");

// What the two calls share.
int check_lstm_common(const Check &c, const void *gates, const float *c_prev, const float *cell_params, const int32_t *clear, int32_t n, int32_t H,
                      int32_t gates_dtype, float eps) {
    if (!gates) return c.bad("null gates");
    if (!c_prev) return c.bad("null c_prev");
    if (!cell_params) return c.bad("null cell_params");
    HS_TRY(c.dtype(gates_dtype, "gates"));
    if (H != 64 && H != 128 && H != 256 && H != 512) return c.bad("hidden must be 64, 128, 256 or 512");
    if (!count_ok(n, {4 * H})) return c.bad("n must be at least 1 and n * 4 * hidden below 2^31");
    if (!std::isfinite(eps) || !(eps > 0.f)) return c.bad("eps must be finite and above 0");
    if (!aligned(4, {c_prev, cell_params, clear})) return c.bad("c_prev, cell_params and clear must be 4-byte aligned");
    if (!aligned(elem_size(gates_dtype), {gates})) return c.bad("gates must be aligned to its element size");
    return HS_OK;
}

int check_lstm(hs_sim *s, const hs_lstm_cell_request *r) {
    const Check c{"hs_lstm_cell"};
    if (!r) return c.bad("null request");
    HS_TRY(check_lstm_common(c, r->gates, r->c_prev, r->cell_params, r->clear, r->n, r->hidden, r->gates_dtype, r->eps));
    if (!r->y && !r->h_next && !r->c_next) return c.bad("every output is null");
    if (r->y) HS_TRY(c.dtype(r->y_dtype, "y"));
    const uintptr_t gsize = elem_size(r->gates_dtype), ysize = elem_size(r->y_dtype);
    if (!aligned(ysize, {r->y}) || !aligned(gsize, {r->h_next})) return c.bad("y and h_next must be aligned to their element size");
    if (!aligned(4, {r->c_next})) return c.bad("c_next must be 4-byte aligned");
    const uintptr_t n = (uintptr_t)r->n, H = (uintptr_t)r->hidden;
    HS_TRY(c.disjoint({range("gates", r->gates, n * 4 * H * gsize), range("c_prev", r->c_prev, n * H * 4),
                       range("cell_params", r->cell_params, HS_LSTM_PARAM_ROWS * H * 4), range("clear", r->clear, n * 4)},
                      {range("y", r->y, n * H * ysize), range("h_next", r->h_next, n * H * gsize), range("c_next", r->c_next, n * H * 4)}));
    return c.handle_ready(s);
}

int check_lstm_bwd(hs_sim *s, const hs_lstm_cell_backward_request *r) {
    const Check c{"hs_lstm_cell_backward"};
    if (!r) return c.bad("null request");
    HS_TRY(check_lstm_common(c, r->gates, r->c_prev, r->cell_params, r->clear, r->n, r->hidden, r->gates_dtype, r->eps));
    if (!r->grad_y) return c.bad("null grad_y");
    if (!r->grad_gates && !r->grad_c_prev && !r->grad_cell_params) return c.bad("every output is null");
    HS_TRY(c.dtype(r->y_dtype, "y"));
    const uintptr_t gsize = elem_size(r->gates_dtype), ysize = elem_size(r->y_dtype);
    if (!aligned(ysize, {r->grad_y}) || !aligned(gsize, {r->grad_h_next, r->grad_gates}))
        return c.bad("grad_y, grad_h_next and grad_gates must be aligned to their element size");
    if (!aligned(4, {r->grad_c_next, r->grad_c_prev, r->grad_cell_params})) return c.bad("grad_c_next, grad_c_prev and grad_cell_params must be 4-byte aligned");
    const uintptr_t n = (uintptr_t)r->n, H = (uintptr_t)r->hidden;
    HS_TRY(c.disjoint({range("gates", r->gates, n * 4 * H * gsize), range("c_prev", r->c_prev, n * H * 4),
                       range("cell_params", r->cell_params, HS_LSTM_PARAM_ROWS * H * 4), range("clear", r->clear, n * 4),
                       range("grad_y", r->grad_y, n * H * ysize), range("grad_h_next", r->grad_h_next, n * H * gsize),
                       range("grad_c_next", r->grad_c_next, n * H * 4)},
                      {range("grad_gates", r->grad_gates, n * 4 * H * gsize), range("grad_c_prev", r->grad_c_prev, n * H * 4),
                       range("grad_cell_params", r->grad_cell_params, HS_LSTM_PARAM_ROWS * H * 4)}));
    return c.handle_ready(s);
}

// One k_lstm_fwd over the rows (the request has passed check_lstm).
int launch_lstm(hs_sim *, hipStream_t strm, const hs_lstm_cell_request *r) {
    hs::LstmArgs a = {};
    a.gates = r->gates; a.cPrev = r->c_prev; a.params = r->cell_params; a.clear = r->clear; a.y = r->y; a.hNext = r->h_next; a.cNext = r->c_next;
    a.n = r->n; a.gatesType = elem_code(r->gates_dtype); a.yType = elem_code(r->y_dtype); a.eps = r->eps;
    const dim3 grid(hs::rows_grid(a.n, hs::kRowsWaves, hs::kRowsMaxGrid)), blk(hs::kRowsThreads);
    with_constant<64, 128, 256, 512>(r->hidden, [&](auto h) { hipLaunchKernelGGL((hs::k_lstm_fwd<decltype(h)::value>), grid, blk, 0, strm, a); });
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// k_lstm_bwd, its parameter sums into the workspace's slices, then their fixed-order sum (the request has passed check_lstm_bwd).
int launch_lstm_bwd(hs_sim *s, hipStream_t strm, const hs_lstm_cell_backward_request *r) {
    hs::LstmBwdArgs a = {};
    a.gates = r->gates; a.cPrev = r->c_prev; a.params = r->cell_params; a.clear = r->clear;
    a.gradY = r->grad_y; a.gradHNext = r->grad_h_next; a.gradCNext = r->grad_c_next;
    a.gradGates = r->grad_gates; a.gradCPrev = r->grad_c_prev; a.workspace = r->grad_cell_params ? s->lstm_partials : nullptr;
    a.n = r->n; a.gatesType = elem_code(r->gates_dtype); a.yType = elem_code(r->y_dtype); a.eps = r->eps;
    const int nparts = hs::rows_grid(a.n, hs::kRowsWaves, hs::kRowsMaxGridBwd), len = hs::kLstmParamRows * r->hidden;
    with_constant<64, 128, 256, 512>(r->hidden, [&](auto h) { hipLaunchKernelGGL((hs::k_lstm_bwd<decltype(h)::value>), dim3(nparts), dim3(hs::kRowsThreads), 0, strm, a); });
    if (r->grad_cell_params) launch_partials_sum<float, hs::kRowsSumCols, hs::kRowsSumSegs>(strm, s->lstm_partials, nparts, len, r->grad_cell_params);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- a dense layer after its GEMM (hs_k_dense.h) ----
namespace {
static_assert(HS_DENSE_PARAM_ROWS == hs::kDenseParamRows && HS_DENSE_MAX_GRID_BWD == hs::kRowsMaxGridBwd && HS_DENSE_MAX_CHANNELS == hs::kDenseMaxC &&
              HS_DENSE_ROWS_PER_ROUND == hs::kRowsWaves, "hs_dense_norm_act_request and k_dense agree");
static_assert(sizeof(hs_dense_norm_act_request) == 48 && offsetof(hs_dense_norm_act_request, params) == 8 && offsetof(hs_dense_norm_act_request, n) == 16 &&
              offsetof(hs_dense_norm_act_request, y_dtype) == 28 && offsetof(hs_dense_norm_act_request, eps) == 32 &&
              offsetof(hs_dense_norm_act_request, slope) == 36 && offsetof(hs_dense_norm_act_request, y) == 40,
              "hs_dense_norm_act_request layout (gpu_hideseek/mlp.py mirrors it)");
static_assert(sizeof(hs_dense_norm_act_backward_request) == 64 && offsetof(hs_dense_norm_act_backward_request, grad_y) == 16 &&
              offsetof(hs_dense_norm_act_backward_request, n) == 24 && offsetof(hs_dense_norm_act_backward_request, y_dtype) == 36 &&
              offsetof(hs_dense_norm_act_backward_request, eps) == 40 && offsetof(hs_dense_norm_act_backward_request, slope) == 44 &&
              offsetof(hs_dense_norm_act_backward_request, grad_z) == 48 && offsetof(hs_dense_norm_act_backward_request, grad_params) == 56,
              "hs_dense_norm_act_backward_request layout (gpu_hideseek/mlp.py mirrors it)");

// What the two calls share.
int check_dense_common(const Check &c, const void *z, const float *params, int32_t n, int32_t C, int32_t z_dtype, float eps, float slope) {
    if (!z) return c.bad("null z");
    if (!params) return c.bad("null params");
    HS_TRY(c.dtype(z_dtype, "z"));
    if (C != 64 && C != 128 && C != 256 && C != 512) return c.bad("channels must be 64, 128, 256 or 512");
    if (!count_ok(n, {C})) return c.bad("n must be at least 1 and n * channels below 2^31");
    if (!std::isfinite(eps) || !(eps > 0.f)) return c.bad("eps must be finite and above 0");
    if (!std::isfinite(slope) || !(slope >= 0.f && slope <= 1.f)) return c.bad("slope must be finite and in [0, 1]");
    if (!aligned(4, {params})) return c.bad("params must be 4-byte aligned");
    if (!aligned(16, {z})) return c.bad("z must be 16-byte aligned");
    return HS_OK;
}

int check_dense(hs_sim *s, const hs_dense_norm_act_request *r) {
    const Check c{"hs_dense_norm_act"};
    if (!r) return c.bad("null request");
    HS_TRY(check_dense_common(c, r->z, r->params, r->n, r->channels, r->z_dtype, r->eps, r->slope));
    if (!r->y) return c.bad("every output is null");
    HS_TRY(c.dtype(r->y_dtype, "y"));
    if (!aligned(16, {r->y})) return c.bad("y must be 16-byte aligned");
    const uintptr_t n = (uintptr_t)r->n, C = (uintptr_t)r->channels;
    HS_TRY(c.disjoint({range("z", r->z, n * C * elem_size(r->z_dtype)), range("params", r->params, HS_DENSE_PARAM_ROWS * C * 4)},
                      {range("y", r->y, n * C * elem_size(r->y_dtype))}));
    return c.handle_ready(s);
}

int check_dense_bwd(hs_sim *s, const hs_dense_norm_act_backward_request *r) {
    const Check c{"hs_dense_norm_act_backward"};
    if (!r) return c.bad("null request");
    HS_TRY(check_dense_common(c, r->z, r->params, r->n, r->channels, r->z_dtype, r->eps, r->slope));
    if (!r->grad_y) return c.bad("null grad_y");
    if (!r->grad_z && !r->grad_params) return c.bad("every output is null");
    HS_TRY(c.dtype(r->y_dtype, "y"));
    if (!aligned(16, {r->grad_y, r->grad_z})) return c.bad("grad_y and grad_z must be 16-byte aligned");
    if (!aligned(4, {r->grad_params})) return c.bad("grad_params must be 4-byte aligned");
    const uintptr_t n = (uintptr_t)r->n, C = (uintptr_t)r->channels, zsize = elem_size(r->z_dtype);
    HS_TRY(c.disjoint({range("z", r->z, n * C * zsize), range("params", r->params, HS_DENSE_PARAM_ROWS * C * 4),
                       range("grad_y", r->grad_y, n * C * elem_size(r->y_dtype))},
                      {range("grad_z", r->grad_z, n * C * zsize), range("grad_params", r->grad_params, HS_DENSE_PARAM_ROWS * C * 4)}));
    return c.handle_ready(s);
}

// One k_dense_fwd over the rows (the request has passed check_dense).
int launch_dense(hs_sim *, hipStream_t strm, const hs_dense_norm_act_request *r) {
    hs::DenseArgs a = {};
    a.z = r->z; a.params = r->params; a.y = r->y;
    a.n = r->n; a.zType = elem_code(r->z_dtype); a.yType = elem_code(r->y_dtype); a.eps = r->eps; a.slope = r->slope;
    const dim3 grid(hs::rows_grid(a.n, hs::kRowsWaves, hs::kRowsMaxGrid)), blk(hs::kRowsThreads);
    with_constant<64, 128, 256, 512>(r->channels, [&](auto ch) { hipLaunchKernelGGL((hs::k_dense_fwd<decltype(ch)::value>), grid, blk, 0, strm, a); });
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// k_dense_bwd, its parameter sums into the workspace's slices, then their fixed-order sum (the request has passed check_dense_bwd).
int launch_dense_bwd(hs_sim *s, hipStream_t strm, const hs_dense_norm_act_backward_request *r) {
    hs::DenseBwdArgs a = {};
    a.z = r->z; a.params = r->params; a.gradY = r->grad_y; a.gradZ = r->grad_z; a.workspace = r->grad_params ? s->dense_partials : nullptr;
    a.n = r->n; a.zType = elem_code(r->z_dtype); a.yType = elem_code(r->y_dtype); a.eps = r->eps; a.slope = r->slope;
    const int nparts = hs::rows_grid(a.n, hs::kRowsWaves, hs::kRowsMaxGridBwd), len = hs::kDenseParamRows * r->channels;
    with_constant<64, 128, 256, 512>(r->channels, [&](auto ch) { hipLaunchKernelGGL((hs::k_dense_bwd<decltype(ch)::value>), dim3(nparts), dim3(hs::kRowsThreads), 0, strm, a); });
    if (r->grad_params) launch_partials_sum<float, hs::kRowsSumCols, hs::kRowsSumSegs>(strm, s->dense_partials, nparts, len, r->grad_params);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the optimiser (hs_k_adam.h) ----
namespace {
static_assert(HS_ADAM_MAX_GRID == hs::kAdamMaxGrid && HS_ADAM_STATE == hs::kAdamState && HS_ADAM_STATS == hs::kAdamStats, "hs_adam_request and k_adam agree");
static_assert(sizeof(hs_adam_request) == 104 && offsetof(hs_adam_request, grads) == 8 && offsetof(hs_adam_request, v) == 24 && offsetof(hs_adam_request, n) == 32 &&
              offsetof(hs_adam_request, lr) == 40 && offsetof(hs_adam_request, weight_decay) == 56 && offsetof(hs_adam_request, max_grad_norm) == 64 &&
              offsetof(hs_adam_request, grad_scale) == 72 && offsetof(hs_adam_request, zero_grad) == 80 && offsetof(hs_adam_request, state) == 88 &&
              offsetof(hs_adam_request, stats) == 96,
              "hs_adam_request layout (gpu_hideseek/optim.py mirrors it)");

// The bytes a request with an accepted n reads and writes: all of them outputs.
std::vector<ByteRange> adam_ranges(const hs_adam_request *r) {
    const uintptr_t bytes = (uintptr_t)r->n * 4;
    return {range("params", r->params, bytes), range("grads", r->grads, bytes), range("m", r->m, bytes), range("v", r->v, bytes),
            range("state", r->state, HS_ADAM_STATE * sizeof(double)), range("stats", r->stats, HS_ADAM_STATS * sizeof(double))};
}

int check_adam(hs_sim *s, const hs_adam_request *r) {
    const Check c{"hs_adam_step"};
    if (!r) return c.bad("null request");
    if (!r->params) return c.bad("null params");
    if (!r->grads) return c.bad("null grads");
    if (!r->m) return c.bad("null m");
    if (!r->v) return c.bad("null v");
    if (!r->state) return c.bad("null state");
    if (r->n < 1 || r->n >= (int64_t)1 << 31) return c.bad("n must be at least 1 and below 2^31");
    if (!aligned(16, {r->params, r->grads, r->m, r->v})) return c.bad("params, grads, m and v must be 16-byte aligned");
    if (!aligned(8, {r->state, r->stats})) return c.bad("state and stats must be 8-byte aligned");
    if (!std::isfinite(r->lr) || !std::isfinite(r->eps) || !std::isfinite(r->weight_decay) || !std::isfinite(r->grad_scale) || !std::isfinite(r->max_grad_norm))
        return c.bad("lr, eps, weight_decay, grad_scale and max_grad_norm must be finite");
    if (!(r->eps > 0.f)) return c.bad("eps must be above 0");
    if (r->lr < 0.f) return c.bad("lr must be at least 0");
    if (r->weight_decay < 0.f) return c.bad("weight_decay must be at least 0");
    if (!(r->grad_scale > 0.0)) return c.bad("grad_scale must be above 0");
    if (!(r->beta1 >= 0.f && r->beta1 < 1.f) || !(r->beta2 >= 0.f && r->beta2 < 1.f)) return c.bad("beta1 and beta2 must be in [0, 1)");
    HS_TRY(c.disjoint(adam_ranges(r), 0));
    return c.handle_ready(s);
}

// k_adam_norm, its partial sums of squares and the snapshot of the state into the workspace, then one k_adam_step over the
// elements (the request has passed check_adam).
hs::AdamArgs adam_args(hs_sim *s, const hs_adam_request *r) {
    hs::AdamArgs a = {};
    a.p = r->params; a.g = r->grads; a.m = r->m; a.v = r->v; a.ws = s->adam_workspace; a.state = r->state; a.stats = r->stats;
    a.n = (int)r->n; a.nparts = hs::adam_grid(a.n, hs::kAdamMaxGrid); a.zeroGrad = r->zero_grad != 0;
    a.lr = r->lr; a.b1 = r->beta1; a.b2 = r->beta2; a.eps = r->eps; a.wd = r->weight_decay;
    a.omb1 = (float)(1.0 - (double)r->beta1); a.omb2 = (float)(1.0 - (double)r->beta2);
    a.gradScale = r->grad_scale; a.maxNorm = r->max_grad_norm;
    return a;
}
int launch_adam(hs_sim *s, hipStream_t strm, const hs_adam_request *r) {
    const hs::AdamArgs a = adam_args(s, r);
    const dim3 blk(hs::kAdamThreads);
    hipLaunchKernelGGL(hs::k_adam_norm<>, dim3(a.nparts), blk, 0, strm, (const float *)r->grads, a.n, (const double *)r->state, s->adam_workspace);
    hipLaunchKernelGGL(hs::k_adam_step<>, dim3(hs::adam_grid(a.n, hs::kAdamStepMaxGrid)), blk, 0, strm, a);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the minibatch gather (hs_k_gather.h) ----
namespace {
static_assert(HS_GATHER_MAX_FIELDS == hs::kGatherMaxFields, "hs_gather_request and k_gather agree");
static_assert(sizeof(hs_gather_field) == 24 && offsetof(hs_gather_field, dst) == 8 && offsetof(hs_gather_field, row_bytes) == 16 &&
              offsetof(hs_gather_field, per_chunk) == 20, "hs_gather_field layout (gpu_hideseek/rollout.py mirrors it)");
static_assert(sizeof(hs_gather_request) == 424 && offsetof(hs_gather_request, m) == 8 && offsetof(hs_gather_request, chunks) == 12 &&
              offsetof(hs_gather_request, chunk_steps) == 16 && offsetof(hs_gather_request, rows) == 20 && offsetof(hs_gather_request, num_fields) == 24 &&
              offsetof(hs_gather_request, bad) == 32 && offsetof(hs_gather_request, fields) == 40,
              "hs_gather_request layout (gpu_hideseek/rollout.py mirrors it)");

// the bytes field i of an accepted request reads and writes
ByteRange gather_src(const hs_gather_request *r, int i) {
    const hs_gather_field &f = r->fields[i];
    return range("src", f.src, (uintptr_t)r->chunks * (f.per_chunk ? 1u : (uintptr_t)r->chunk_steps) * (uintptr_t)r->rows * (uintptr_t)f.row_bytes);
}
ByteRange gather_dst(const hs_gather_request *r, int i) {
    const hs_gather_field &f = r->fields[i];
    return range("dst", f.dst, (f.per_chunk ? 1u : (uintptr_t)r->chunk_steps) * (uintptr_t)r->m * (uintptr_t)f.row_bytes);
}

int check_gather(hs_sim *s, const hs_gather_request *r) {
    const Check c{"hs_gather_sequences"};
    if (!r) return c.bad("null request");
    if (!r->index) return c.bad("null index");
    if (r->m < 1 || r->chunks < 1 || r->chunk_steps < 1 || r->rows < 1) return c.bad("m, chunks, chunk_steps and rows must be at least 1");
    if ((int64_t)r->chunks * r->rows >= (int64_t)1 << 31) return c.bad("chunks * rows must stay below 2^31");
    if (r->num_fields < 1 || r->num_fields > HS_GATHER_MAX_FIELDS) return c.bad("num_fields must be in [1, HS_GATHER_MAX_FIELDS]");
    if ((int64_t)(r->num_fields + 1) * r->m >= (int64_t)1 << 31) return c.bad("(num_fields + 1) * m must stay below 2^31");
    if (!aligned(4, {r->index, r->bad})) return c.bad("index and bad must be 4-byte aligned");
    for (int i = 0; i < r->num_fields; ++i) {
        const hs_gather_field &f = r->fields[i];
        const std::string which = "field " + std::to_string(i);
        if (!f.src || !f.dst) return c.bad(which + ": null src or dst");
        if (f.row_bytes < 4 || f.row_bytes > HS_GATHER_MAX_ROW_BYTES || f.row_bytes % 4) return c.bad(which + ": row_bytes must be a multiple of 4 in [4, HS_GATHER_MAX_ROW_BYTES]");
        if (!aligned(4, {f.src, f.dst})) return c.bad(which + ": src and dst must be 4-byte aligned");
    }
    // no output (a dst, bad) overlaps an input (a src, index) or an earlier output
    const ByteRange index = range("index", r->index, (uintptr_t)r->m * 4), bad = range("bad", r->bad, 4);
    for (int i = 0; i <= r->num_fields; ++i) {
        const ByteRange o = i < r->num_fields ? gather_dst(r, i) : bad;
        const std::string which = i < r->num_fields ? "field " + std::to_string(i) + ": dst" : std::string("bad");
        if (overlap(o, index)) return c.bad(which + " overlaps index");
        for (int k = 0; k < r->num_fields; ++k)
            if (overlap(o, gather_src(r, k))) return c.bad(which + " overlaps the src of field " + std::to_string(k));
        for (int k = 0; k < i; ++k)
            if (overlap(o, gather_dst(r, k))) return c.bad(which + " overlaps the dst of field " + std::to_string(k));
    }
    return c.handle_ready(s);
}

// bad zeroed, then one k_gather over every field (the request has passed check_gather): the fields that move as 16-byte
// pieces first, in the request's order, then the others.
int launch_gather(hs_sim *, hipStream_t strm, const hs_gather_request *r) {
    hs::GatherArgs a = {};
    const auto wide = [](const hs_gather_field &f) { return f.row_bytes % hs::kGatherVec == 0 && aligned(hs::kGatherVec, {f.src, f.dst}); };
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i < r->num_fields; ++i)
            if (wide(r->fields[i]) == (pass == 0))
                a.f[a.nFields++] = {(const char *)r->fields[i].src, (char *)r->fields[i].dst, r->fields[i].row_bytes, r->fields[i].per_chunk != 0};
        if (pass == 0) a.nWide = a.nFields;
    }
    a.index = r->index; a.bad = r->bad; a.m = r->m; a.L = r->chunk_steps; a.n = r->rows; a.total = r->chunks * r->rows;
    a.units = (uint32_t)(a.nWide + (a.nFields > a.nWide ? 1 : 0)) * (uint32_t)r->m;
    if (r->bad) HS_HIP(hipMemsetAsync(r->bad, 0, sizeof(int32_t), strm));
    const uint32_t blocks = (a.units + hs::kGatherWaves - 1) / hs::kGatherWaves;
    hipLaunchKernelGGL(hs::k_gather<>, dim3(blocks < (uint32_t)hs::kGatherMaxGrid ? blocks : hs::kGatherMaxGrid), dim3(hs::kGatherThreads), 0, strm, a);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- episode statistics (hs_k_episode.h) ----
namespace {
static_assert(HS_EPISODE_STATS == hs::kEpiStats && HS_EPISODE_SIDE_STATS == hs::kEpiSide && HS_EPISODE_OUT == hs::kEpiOut &&
              HS_EPISODE_TRACKED == hs::kEpiTracked && HS_EPISODE_WAITING == hs::kEpiWaiting && 2 * hs::kEpiSide == hs::kEpiHiderWins &&
              hs::kEpiWorldEpisodes == hs::kEpiStats - 1, "hs_episode_request and k_episode agree");
static_assert(sizeof(hs_episode_request) == 128 && offsetof(hs_episode_request, gamma) == 48 && offsetof(hs_episode_request, ret) == 56 &&
              offsetof(hs_episode_request, len) == 80 && offsetof(hs_episode_request, world_hider_team) == 104 && offsetof(hs_episode_request, table) == 120,
              "hs_episode_request layout (gpu_hideseek/episodes.py mirrors it)");
static_assert(kExports[HS_EXPORT_SELF_TYPE].dtype == HS_DTYPE_I32 && kExports[HS_EXPORT_SELF_TYPE].per_agent && kExports[HS_EXPORT_SELF_TYPE].tail[0] == 1 &&
              kExports[HS_EXPORT_REWARD].tail[0] == 1 && kExports[HS_EXPORT_DONE].tail[0] == 1 && kExports[HS_EXPORT_SELF_MASK].tail[0] == 1 &&
              kExports[HS_EXPORT_EPISODE_RESULT].dtype == HS_DTYPE_F32 && !kExports[HS_EXPORT_EPISODE_RESULT].per_agent &&
              kExports[HS_EXPORT_EPISODE_RESULT].tail[0] == 2 && hs::AGENT_SEEKER == 0 && hs::AGENT_HIDER == 1,
              "k_episode reads the reward, done, self_type, self_mask and episode_result exports");
static_assert(hs::kEpiThreads >= hs::kMaxAgents && hs::kEpiStats * hs::kEpiSumSegs <= 1024, "a workgroup of k_episode holds a world, k_episode_fold is one workgroup");

// The request with every null input replaced by the handle's own (the state and the table are left as given).
hs::EpisodeArgs episode_args(const hs_sim *s, const hs_episode_request *r) {
    const hs::SimState &S = s->S;
    return {r->reward ? r->reward : S.xReward, r->done ? r->done : S.xDone, r->self_type ? r->self_type : S.xSelfType,
            r->self_mask ? r->self_mask : S.xSelfMask, r->episode_result ? r->episode_result : S.xEpisodeResult, r->hider_team, S.counts,
            r->ret, r->disc, r->gpow, r->len, r->type, r->phase, r->world_hider_team, r->world_phase, s->episode_partials, S.N, s->A, r->gamma};
}

int check_episode(hs_sim *s, const hs_episode_request *r) {
    const Check c{"hs_episode_stats"};
    if (!r) return c.bad("null request");
    if (!r->ret || !r->disc || !r->gpow || !r->len || !r->type || !r->phase || !r->world_hider_team || !r->world_phase) return c.bad("null state pointer");
    if (!r->table) return c.bad("null table");
    if (!(r->gamma >= 0.f && r->gamma <= 1.f)) return c.bad("gamma must be finite and in [0, 1]");
    if (!aligned(4, {r->reward, r->done, r->self_type, r->self_mask, r->episode_result, r->hider_team, r->ret, r->disc, r->gpow, r->len, r->type, r->phase,
                     r->world_hider_team, r->world_phase}))
        return c.bad("every input and state pointer must be 4-byte aligned");
    if (!aligned(8, {r->table})) return c.bad("table must be 8-byte aligned");
    if ((s->S.flags & hs::FLAG_EXT_SKIP_OBSERVATIONS) && (!r->self_type || !r->self_mask))
        return c.bad("a null self_type or self_mask needs the exports that HS_FLAG_EXT_SKIP_OBSERVATIONS leaves unwritten after a reset", HS_ERR_UNSUPPORTED);
    const hs::EpisodeArgs a = episode_args(s, r);
    const uintptr_t worlds = (uintptr_t)s->S.N, rows = worlds * (uintptr_t)s->A;
    HS_TRY(c.disjoint({range("reward", a.reward, rows * 4), range("done", a.done, rows * 4), range("self_type", a.selfType, rows * 4),
                       range("self_mask", a.selfMask, rows * 4), range("episode_result", a.episodeResult, worlds * 8), range("hider_team", a.hiderTeam, worlds * 4)},
                      {range("ret", r->ret, rows * 4), range("disc", r->disc, rows * 4), range("gpow", r->gpow, rows * 4), range("len", r->len, rows * 4),
                       range("type", r->type, rows * 4), range("phase", r->phase, rows * 4), range("world_hider_team", r->world_hider_team, worlds * 4),
                       range("world_phase", r->world_phase, worlds * 4), range("table", r->table, HS_EPISODE_STATS * sizeof(double))}));
    return c.handle_ready(s);
}
// One k_episode over every agent row (the request has passed check_episode), then the fixed-order add onto the table.
int launch_episode(hs_sim *s, hipStream_t strm, const hs_episode_request *r) {
    const hs::EpisodeArgs a = episode_args(s, r);
    const int grid = hs::episode_grid(a.worlds, a.A);
    hipLaunchKernelGGL(hs::k_episode<>, dim3(grid), dim3(hs::kEpiThreads), 0, strm, a);
    hipLaunchKernelGGL(hs::k_episode_fold<>, dim3(1), dim3(hs::kEpiStats * hs::kEpiSumSegs), 0, strm, (const double *)s->episode_partials, grid, r->table);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the league (hs_k_league.h) ----
namespace {
static_assert(HS_LEAGUE_MAX_POLICIES == hs::kLeagueMaxPolicies && HS_LEAGUE_OUTCOMES == hs::kLeagueOutcomes && HS_LEAGUE_HIDERS_WIN == hs::kLeagueHidersWin &&
              HS_LEAGUE_SEEKERS_WIN == hs::kLeagueSeekersWin && HS_LEAGUE_DRAW == hs::kLeagueDraw && HS_LEAGUE_NO_OUTCOME == hs::kLeagueNoOutcome,
              "hs_league_request and k_league agree");
static_assert(sizeof(hs_league_request) == 128 && offsetof(hs_league_request, num_policies) == 40 && offsetof(hs_league_request, team_size) == 44 &&
              offsetof(hs_league_request, k_factor) == 48 && offsetof(hs_league_request, policy_assignments) == 56 && offsetof(hs_league_request, slot) == 64 &&
              offsetof(hs_league_request, world_hider_team) == 88 && offsetof(hs_league_request, bad) == 104 && offsetof(hs_league_request, counts) == 112 &&
              offsetof(hs_league_request, elo) == 120,
              "hs_league_request layout (gpu_hideseek/league.py mirrors it)");
static_assert(kExports[HS_EXPORT_AGENT_POLICY].dtype == HS_DTYPE_I32 && kExports[HS_EXPORT_AGENT_POLICY].per_agent && kExports[HS_EXPORT_AGENT_POLICY].tail[0] == 1 &&
              kExports[HS_EXPORT_SELF_TYPE].dtype == HS_DTYPE_I32 && kExports[HS_EXPORT_SELF_TYPE].tail[0] == 1 && kExports[HS_EXPORT_DONE].dtype == HS_DTYPE_I32 &&
              kExports[HS_EXPORT_DONE].tail[0] == 1 && kExports[HS_EXPORT_SELF_MASK].dtype == HS_DTYPE_F32 && kExports[HS_EXPORT_SELF_MASK].tail[0] == 1 &&
              kExports[HS_EXPORT_EPISODE_RESULT].dtype == HS_DTYPE_F32 && kExports[HS_EXPORT_EPISODE_RESULT].tail[0] == 2,
              "k_league reads the done, self_type, self_mask and episode_result exports and writes policy_assignments");
static_assert(HS_LEAGUE_MAX_GROUP == hs::kLeagueMaxGroup, "a schedule table holds every ordered pair");
static_assert(hs::kLeagueThreads >= hs::kMaxAgents && hs::kLeagueMaxPolicies * hs::kLeagueMaxPolicies <= 1024, "a workgroup of k_league holds a world, k_league_fold is one workgroup");

// The request with every null input, and a null policy_assignments, replaced by the handle's own.
hs::LeagueArgs league_args(const hs_sim *s, const hs_league_request *r) {
    const hs::SimState &S = s->S;
    return {r->done ? r->done : S.xDone, r->self_type ? r->self_type : S.xSelfType, r->self_mask ? r->self_mask : S.xSelfMask,
            r->episode_result ? r->episode_result : S.xEpisodeResult, r->hider_team, S.counts,
            r->policy_assignments ? r->policy_assignments : S.xPolicy, r->slot, r->row_of_slot, r->clear_slot, r->world_hider_team, r->world_phase,
            s->league_step, S.N, s->A, r->num_policies, r->team_size};
}

// hs_league_step and, with `scheduled`, hs_league_step_scheduled: one set of rules, of which only the schedule's differ.
int check_league_as(const Check &c, hs_sim *s, const hs_league_request *r, bool scheduled) {
    if (!r) return c.bad("null request");
    if (!r->world_hider_team || !r->world_phase) return c.bad("null state pointer");
    if (!r->counts) return c.bad("null counts");
    if (!r->elo) return c.bad("null elo");
    if (r->num_policies < 1 || r->num_policies > HS_LEAGUE_MAX_POLICIES) return c.bad("num_policies must be in [1, HS_LEAGUE_MAX_POLICIES]");
    if (r->team_size < 1 || s->A != 2 * r->team_size) return c.bad("team_size must be at least 1 and the handle's agents per world 2 * team_size");
    const int64_t P = r->num_policies;
    if (scheduled) {
        if (s->league_group == 0) return c.bad("no schedule is set (hs_league_set_schedule)");
        if (r->num_policies != s->league_policies) return c.bad("num_policies must equal the schedule's");
        if ((int64_t)s->S.N % s->league_group) return c.bad("the number of worlds must be a multiple of the schedule's group");
    } else if ((int64_t)s->S.N % (P * P)) {
        return c.bad("the number of worlds must be a multiple of num_policies^2");
    }
    if ((int64_t)s->S.N * s->A >= (int64_t)1 << 31) return c.bad("worlds * agents must stay below 2^31");
    if (!std::isfinite(r->k_factor) || !(r->k_factor > 0.0)) return c.bad("k_factor must be finite and above 0");
    if (!aligned(4, {r->done, r->self_type, r->self_mask, r->episode_result, r->hider_team, r->policy_assignments, r->slot, r->row_of_slot, r->clear_slot,
                     r->world_hider_team, r->world_phase, r->bad}))
        return c.bad("every input, routing and state pointer must be 4-byte aligned");
    if (!aligned(8, {r->counts, r->elo})) return c.bad("counts and elo must be 8-byte aligned");
    if ((s->S.flags & hs::FLAG_EXT_SKIP_OBSERVATIONS) && (!r->self_type || !r->self_mask))
        return c.bad("a null self_type or self_mask needs the exports that HS_FLAG_EXT_SKIP_OBSERVATIONS leaves unwritten after a reset", HS_ERR_UNSUPPORTED);
    const hs::LeagueArgs a = league_args(s, r);
    const uintptr_t worlds = (uintptr_t)s->S.N, rows = worlds * (uintptr_t)s->A;
    HS_TRY(c.disjoint({range("done", a.done, rows * 4), range("self_type", a.selfType, rows * 4), range("self_mask", a.selfMask, rows * 4),
                       range("episode_result", a.episodeResult, worlds * 8), range("hider_team", a.hiderTeam, worlds * 4)},
                      {range("policy_assignments", a.policy, rows * 4), range("slot", r->slot, rows * 4), range("row_of_slot", r->row_of_slot, rows * 4),
                       range("clear_slot", r->clear_slot, rows * 4), range("world_hider_team", r->world_hider_team, worlds * 4),
                       range("world_phase", r->world_phase, worlds * 4), range("bad", r->bad, 4),
                       range("counts", r->counts, (uintptr_t)(P * P) * HS_LEAGUE_OUTCOMES * sizeof(int64_t)), range("elo", r->elo, (uintptr_t)P * sizeof(double))}));
    return c.handle_ready(s);
}
int check_league(hs_sim *s, const hs_league_request *r) { return check_league_as(Check{"hs_league_step"}, s, r, false); }
int check_league_scheduled(hs_sim *s, const hs_league_request *r) { return check_league_as(Check{"hs_league_step_scheduled"}, s, r, true); }
// The fold of the step's counts and ratings, after either kernel over the rows.
int launch_league_fold(hs_sim *s, hipStream_t strm, const hs_league_request *r) {
    hipLaunchKernelGGL(hs::k_league_fold<>, dim3(1), dim3(hs::kLeagueMaxPolicies * hs::kLeagueMaxPolicies), 0, strm, s->league_step, r->num_policies, r->k_factor,
                       (long long *)r->counts, r->elo, r->bad);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
// One k_league over every agent row (the request has passed check_league), then the fold.
int launch_league(hs_sim *s, hipStream_t strm, const hs_league_request *r) {
    const hs::LeagueArgs a = league_args(s, r);
    hipLaunchKernelGGL(hs::k_league<>, dim3(hs::league_grid(a.worlds, a.A)), dim3(hs::kLeagueThreads), 0, strm, a);
    return launch_league_fold(s, strm, r);
}
// The same with the handle's schedule table (the request has passed check_league_scheduled).
int launch_league_scheduled(hs_sim *s, hipStream_t strm, const hs_league_request *r) {
    const hs::LeagueArgs a = league_args(s, r);
    hipLaunchKernelGGL(hs::k_league_scheduled<>, dim3(hs::league_grid(a.worlds, a.A)), dim3(hs::kLeagueThreads), 0, strm, a, (const int4 *)s->league_table,
                       s->league_group, s->league_sides);
    return launch_league_fold(s, strm, r);
}

// hs_league_set_schedule: the rules of a table, then its device form.  Nothing of the handle changes before every rule has passed.
int set_league_schedule(hs_sim *s, const int32_t *pairs, int32_t group, int32_t num_policies) {
    const Check c{"hs_league_set_schedule"};
    HS_TRY(c.handle_ready(s));
    if (group == 0) { s->league_group = s->league_sides = s->league_policies = 0; return HS_OK; }
    if (num_policies < 1 || num_policies > HS_LEAGUE_MAX_POLICIES) return c.bad("num_policies must be in [1, HS_LEAGUE_MAX_POLICIES]");
    if (group < 0 || group > HS_LEAGUE_MAX_GROUP) return c.bad("group must be 0 (no schedule) or in [1, HS_LEAGUE_MAX_GROUP]");
    if (!pairs) return c.bad("null pairs");
    const int N = num_policies, G = group;
    int sides[HS_LEAGUE_MAX_POLICIES] = {};
    std::vector<int4> table((size_t)G);
    for (int q = 0; q < G; ++q) {
        const int32_t i = pairs[2 * q], j = pairs[2 * q + 1];
        if (i < 0 || i >= N || j < 0 || j >= N) return c.bad("pairs[" + std::to_string(q) + "] is out of range: every entry must be in [0, num_policies)");
        table[(size_t)q] = make_int4(i, j, sides[i], sides[j]);
        ++sides[i]; ++sides[j];
    }
    for (int p = 0; p < N; ++p)
        if (sides[p] * N != 2 * G) return c.bad("the schedule is not regular: every policy must hold the same number 2 group / num_policies of sides");
    HS_HIP(hipMemcpy(s->league_table, table.data(), table.size() * sizeof(int4), hipMemcpyHostToDevice));
    HS_HIP(hipDeviceSynchronize());       // the table is in place, whatever stream the next step is enqueued on
    s->league_group = G; s->league_sides = 2 * G / N; s->league_policies = N;
    return HS_OK;
}
}  // namespace

// ---- the routed pack (hs_k_pack_routed.h) ----
namespace {
static_assert(sizeof(hs_pack_routed_request) == 80 && offsetof(hs_pack_routed_request, actor_dtype) == 8 && offsetof(hs_pack_routed_request, critic) == 16 &&
              offsetof(hs_pack_routed_request, critic_dtype) == 24 && offsetof(hs_pack_routed_request, row_of_slot) == 32 &&
              offsetof(hs_pack_routed_request, num_policies) == 40 && offsetof(hs_pack_routed_request, tables) == 48 &&
              offsetof(hs_pack_routed_request, moments) == 56 && offsetof(hs_pack_routed_request, moments_stride) == 64 && offsetof(hs_pack_routed_request, bad) == 72,
              "hs_pack_routed_request layout (gpu_hideseek/policy_inputs.py mirrors it)");
static_assert(hs::kLeagueMaxPolicies <= hs::kPackMaxGrid, "every policy has a workgroup");

int check_pack_routed(hs_sim *s, const hs_pack_routed_request *r) {
    const Check c{"hs_pack_policy_inputs_routed"};
    if (!r) return c.bad("null request");
    if (s->S.flags & hs::FLAG_EXT_SKIP_OBSERVATIONS) return c.bad("HS_FLAG_EXT_SKIP_OBSERVATIONS leaves no observations to pack", HS_ERR_UNSUPPORTED);
    HS_TRY(c.handle_ready(s));
    if (!r->actor && !r->critic && !r->moments) return c.bad("every output is null");
    if (r->actor) HS_TRY(c.dtype(r->actor_dtype, "output"));
    if (r->critic) HS_TRY(c.dtype(r->critic_dtype, "output"));
    if (!r->row_of_slot) return c.bad("null row_of_slot");
    const int64_t R = (int64_t)s->S.N * s->A;
    if (r->num_policies < 1 || r->num_policies > HS_LEAGUE_MAX_POLICIES) return c.bad("num_policies must be in [1, HS_LEAGUE_MAX_POLICIES]");
    if (R % r->num_policies) return c.bad("the number of agent rows must be a multiple of num_policies");
    if (r->moments && r->moments_stride < HS_PACK_MOMENTS) return c.bad("moments_stride must be at least HS_PACK_MOMENTS");
    if (!aligned(16, {r->actor, r->critic})) return c.bad("outputs must be 16-byte aligned");
    if (!aligned(16, {r->tables})) return c.bad("tables must be 16-byte aligned");
    if (!aligned(8, {r->moments})) return c.bad("moments must be 8-byte aligned");
    if (!aligned(4, {r->row_of_slot, r->bad})) return c.bad("row_of_slot and bad must be 4-byte aligned");
    const uintptr_t N = (uintptr_t)r->num_policies, rows = (uintptr_t)R;
    return c.disjoint({range("row_of_slot", r->row_of_slot, rows * 4), range("tables", r->tables, N * HS_NORM_TABLE * sizeof(float))},
                      {range("actor", r->actor, rows * HS_PACK_ROW * elem_size(r->actor_dtype)), range("critic", r->critic, rows * HS_PACK_ROW * elem_size(r->critic_dtype)),
                       range("moments", r->moments, r->moments ? ((N - 1) * (uintptr_t)r->moments_stride + HS_PACK_MOMENTS) * sizeof(double) : 0), range("bad", r->bad, 4)});
}
// The fixed-order sum of every policy's G workspace rows, after a k_pack_routed that wrote them.  A template, as
// launch_pack_moments_sum is and for its reason: k_partials_sum stays where launch_pack's instantiates it.
template <int kSegs = hs::kPackSumSegs>
int launch_pack_routed_sums(hs_sim *s, hipStream_t strm, const hs_pack_routed_request *r, int G) {
    if (r->moments)
        for (int p = 0; p < r->num_policies; ++p)
            launch_partials_sum<double, hs::kPackThreads / kSegs, kSegs>(strm, s->pack_routed_partials + (size_t)p * G * hs::kPackMoments, G, hs::kPackMoments,
                                                                         r->moments + (size_t)p * r->moments_stride);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
// bad zeroed, one k_pack_routed over every slot (the request has passed check_pack_routed), then the fixed-order sum of each
// policy's moments.  With no rows requested the table is not read.
int launch_pack_routed(hs_sim *s, hipStream_t strm, const hs_pack_routed_request *r) {
    const hs_pack_request plain = {r->actor, r->actor_dtype, r->critic, r->critic_dtype, r->moments};
    hs::PackRoutedArgs a = {pack_args(s, &plain), r->row_of_slot, r->tables, r->bad, 0};
    a.p.partials = s->pack_routed_partials;
    a.perPolicy = a.p.rows / r->num_policies;
    const int G = hs::pack_routed_grid(a.perPolicy, r->num_policies);
    const dim3 grid(G, r->num_policies), blk(hs::kPackThreads);
    const bool norm = r->tables && (r->actor || r->critic);
    if (r->bad) HS_HIP(hipMemsetAsync(r->bad, 0, sizeof(int32_t), strm));
    with_pack_type(r->actor, r->actor_dtype, [&](auto ta) {
        with_pack_type(r->critic, r->critic_dtype, [&](auto tc) {
            typedef decltype(ta) TA;
            typedef decltype(tc) TC;
            constexpr bool rows = !(std::is_same<TA, hs::PackAbsent>::value && std::is_same<TC, hs::PackAbsent>::value);
            if constexpr (rows) {
                if (r->moments && norm) hipLaunchKernelGGL((hs::k_pack_routed<TA, TC, true, true>), grid, blk, 0, strm, a);
                else if (r->moments) hipLaunchKernelGGL((hs::k_pack_routed<TA, TC, true, false>), grid, blk, 0, strm, a);
                else if (norm) hipLaunchKernelGGL((hs::k_pack_routed<TA, TC, false, true>), grid, blk, 0, strm, a);
                else hipLaunchKernelGGL((hs::k_pack_routed<TA, TC, false, false>), grid, blk, 0, strm, a);
            } else {
                hipLaunchKernelGGL((hs::k_pack_routed<TA, TC, true, false>), grid, blk, 0, strm, a);       // the moments alone (check_pack_routed)
            }
        });
    });
    return launch_pack_routed_sums<>(s, strm, r, G);
}
}  // namespace

// ---- the routed sampler (hs_k_sample_routed.h) ----
namespace {
static_assert(sizeof(hs_sample_routed_request) == 112 && offsetof(hs_sample_routed_request, logits_stride) == 12 && offsetof(hs_sample_routed_request, buckets) == 16 &&
              offsetof(hs_sample_routed_request, mode) == 36 && offsetof(hs_sample_routed_request, seed) == 44 && offsetof(hs_sample_routed_request, counter) == 52 &&
              offsetof(hs_sample_routed_request, row_of_slot) == 56 && offsetof(hs_sample_routed_request, action_rows) == 64 &&
              offsetof(hs_sample_routed_request, action) == 72 && offsetof(hs_sample_routed_request, head_log_prob) == 96 && offsetof(hs_sample_routed_request, bad) == 104,
              "hs_sample_routed_request layout (gpu_hideseek/action_sampling.py mirrors it)");

int check_sample_routed(hs_sim *s, const hs_sample_routed_request *r) {
    const Check c{"hs_sample_actions_routed"};
    if (!r) return c.bad("null request");
    if (!r->logits) return c.bad("null logits");
    if (!r->row_of_slot) return c.bad("null row_of_slot");
    HS_TRY(c.dtype(r->logits_dtype, "logits"));
    if (r->mode != HS_SAMPLE_DRAW && r->mode != HS_SAMPLE_GREEDY) return c.bad("mode must be HS_SAMPLE_DRAW or HS_SAMPLE_GREEDY");
    if (r->flags) return c.bad("flags must be 0");
    int L;
    HS_TRY(c.buckets(r->buckets, &L));
    if (r->logits_stride < L) return c.bad("logits_stride is below the sum of the buckets");
    if (!aligned(elem_size(r->logits_dtype), {r->logits})) return c.bad("logits must be aligned to their element size");
    if (!aligned(4, {r->row_of_slot, r->action_rows, r->action, r->log_prob, r->entropy, r->head_log_prob, r->bad}))
        return c.bad("row_of_slot, action_rows, action, log_prob, entropy, head_log_prob and bad must be 4-byte aligned");
    if (r->action_rows && !r->action && !r->log_prob && !r->entropy && !r->head_log_prob)
        return c.bad("every slot-order output is null and action_rows is given: hs_sample_actions on the gathered logits does that");
    HS_TRY(c.handle_ready(s));
    const uintptr_t rows = (uintptr_t)s->S.N * (uintptr_t)s->A;
    if ((int64_t)rows * r->logits_stride >= (int64_t)1 << 31) return c.bad("rows * logits_stride must stay below 2^31");
    return c.disjoint({range("logits", r->logits, ((rows - 1) * (uintptr_t)r->logits_stride + (uintptr_t)L) * elem_size(r->logits_dtype)),
                       range("row_of_slot", r->row_of_slot, rows * 4)},
                      {range("action_rows", r->action_rows ? r->action_rows : s->S.xAction, rows * HS_SAMPLE_HEADS * 4),
                       range("action", r->action, rows * HS_SAMPLE_HEADS * 4), range("log_prob", r->log_prob, rows * 4), range("entropy", r->entropy, rows * 4),
                       range("head_log_prob", r->head_log_prob, rows * HS_SAMPLE_HEADS * 4), range("bad", r->bad, 4)});
}
// bad zeroed, then one k_sample_routed over every slot (the request has passed check_sample_routed).
int launch_sample_routed(hs_sim *s, hipStream_t strm, const hs_sample_routed_request *r) {
    const hs::SimState &S = s->S;
    hs::SampleRoutedArgs a = {};
    a.s.logits = r->logits;
    a.s.action = r->action_rows ? r->action_rows : S.xAction;
    a.s.logProb = r->log_prob; a.s.entropy = r->entropy; a.s.headLogProb = r->head_log_prob;
    a.s.L = pack_buckets(r->buckets, &a.s.bucketK, &a.s.bucketOff);
    a.s.rows = S.N * s->A; a.s.stride = r->logits_stride; a.s.mode = r->mode;
    a.s.seed0 = r->seed[0]; a.s.seed1 = r->seed[1]; a.s.counter = r->counter;
    a.s.row0Global = (uint32_t)S.worldOffset * (uint32_t)s->A;
    a.rowOfSlot = r->row_of_slot; a.actionSlots = r->action; a.bad = r->bad;
    if (r->bad) HS_HIP(hipMemsetAsync(r->bad, 0, sizeof(int32_t), strm));
    const dim3 grid(hs::sample_grid(a.s.rows)), blk(hs::kSampleThreads);
    with_elem(r->logits_dtype, [&](auto t) { hipLaunchKernelGGL(hs::k_sample_routed<decltype(t)>, grid, blk, 0, strm, a); });
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- grouped advantages (hs_k_gae.h) ----
namespace {
static_assert(sizeof(hs_gae_grouped_request) == 88 && offsetof(hs_gae_grouped_request, groups) == 80, "hs_gae_grouped_request layout (gpu_hideseek/advantages.py mirrors it)");

int check_gae_grouped(hs_sim *s, const hs_gae_grouped_request *r) {
    const Check c{"hs_compute_gae_grouped"};
    if (!r) return c.bad("null request");
    if (r->groups < 1 || r->groups > HS_LEAGUE_MAX_POLICIES) return c.bad("groups must be in [1, HS_LEAGUE_MAX_POLICIES]");
    if (((int64_t)s->S.N * s->A) % r->groups) return c.bad("the number of agent rows must be a multiple of groups");
    return check_gae_request(c, s, &r->gae, r->groups);
}
// One k_gae_grouped over every agent row (the request has passed check_gae_grouped), then the fixed-order sum of each
// group's moments: k_partials_sum as launch_gae instantiates it.
int launch_gae_grouped(hs_sim *s, hipStream_t strm, const hs_gae_grouped_request *g) {
    const hs_gae_request *r = &g->gae;
    const int rows = s->S.N * s->A, m = rows / g->groups, parts = hs::gae_grid(m);
    const hs::GaeGroupedArgs a = {{r->reward, r->done, r->value, r->bootstrap, r->mask, r->advantage, r->returns,
                                   r->moments ? s->gae_partials : nullptr, rows, r->steps, r->gamma, r->lambda}, m};
    const dim3 grid(parts, g->groups), blk(hs::kGaeThreads);
    with_elem(r->value_dtype, [&](auto t) { hipLaunchKernelGGL(hs::k_gae_grouped<decltype(t)>, grid, blk, 0, strm, a); });
    if (r->moments)
        for (int q = 0; q < g->groups; ++q)
            launch_partials_sum<double, hs::kGaeMoments, hs::kGaeSumSegs>(strm, s->gae_partials + (size_t)q * parts * hs::kGaeMoments, parts, hs::kGaeMoments,
                                                                          r->moments + (size_t)q * hs::kGaeMoments);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the attention core of the entity self-attention encoder (hs_k_attend.h) ----
namespace {
static_assert(HS_ATTEND_TOKENS == hs::kAttendTokens && HS_ATTEND_HEADS == hs::kAttendHeads && HS_ATTEND_ROWS_PER_ROUND == hs::kRowsWaves &&
              HS_ATTEND_MAX_GRID == hs::kRowsMaxGrid, "hs_entity_attend_request and k_attend agree");
static_assert(sizeof(hs_entity_attend_request) == 40 && offsetof(hs_entity_attend_request, key_mask) == 8 && offsetof(hs_entity_attend_request, n) == 16 &&
              offsetof(hs_entity_attend_request, out_dtype) == 28 && offsetof(hs_entity_attend_request, out) == 32,
              "hs_entity_attend_request layout (gpu_hideseek/entity_attention.py mirrors it)");
static_assert(sizeof(hs_entity_attend_backward_request) == 48 && offsetof(hs_entity_attend_backward_request, grad_out) == 16 &&
              offsetof(hs_entity_attend_backward_request, n) == 24 && offsetof(hs_entity_attend_backward_request, grad_dtype) == 36 &&
              offsetof(hs_entity_attend_backward_request, grad_qkv) == 40,
              "hs_entity_attend_backward_request layout (gpu_hideseek/entity_attention.py mirrors it)");

// What the two calls share.
int check_attend_common(const Check &c, const void *qkv, int32_t n, int32_t E, int32_t qkv_dtype) {
    if (!qkv) return c.bad("null qkv");
    HS_TRY(c.dtype(qkv_dtype, "qkv"));
    if (E != 64 && E != 128) return c.bad("embed_dim must be 64 or 128");
    if (n < 1 || n >= HS_ATTEND_MAX_ROWS) return c.bad("n must be at least 1 and below HS_ATTEND_MAX_ROWS");
    if (!aligned(16, {qkv})) return c.bad("qkv must be 16-byte aligned");
    return HS_OK;
}

int check_attend(hs_sim *s, const hs_entity_attend_request *r) {
    const Check c{"hs_entity_attend"};
    if (!r) return c.bad("null request");
    HS_TRY(check_attend_common(c, r->qkv, r->n, r->embed_dim, r->qkv_dtype));
    if (!r->out) return c.bad("null out");
    HS_TRY(c.dtype(r->out_dtype, "out"));
    if (!aligned(16, {r->out})) return c.bad("out must be 16-byte aligned");
    const uintptr_t n = (uintptr_t)r->n, SE = (uintptr_t)HS_ATTEND_TOKENS * r->embed_dim;
    HS_TRY(c.disjoint({range("qkv", r->qkv, n * 3 * SE * elem_size(r->qkv_dtype)), range("key_mask", r->key_mask, n * HS_ATTEND_TOKENS)},
                      {range("out", r->out, n * SE * elem_size(r->out_dtype))}));
    return c.handle_ready(s);
}

int check_attend_bwd(hs_sim *s, const hs_entity_attend_backward_request *r) {
    const Check c{"hs_entity_attend_backward"};
    if (!r) return c.bad("null request");
    HS_TRY(check_attend_common(c, r->qkv, r->n, r->embed_dim, r->qkv_dtype));
    if (!r->grad_out) return c.bad("null grad_out");
    if (!r->grad_qkv) return c.bad("null grad_qkv");
    HS_TRY(c.dtype(r->grad_dtype, "grad"));
    if (!aligned(16, {r->grad_out, r->grad_qkv})) return c.bad("grad_out and grad_qkv must be 16-byte aligned");
    const uintptr_t n = (uintptr_t)r->n, SE = (uintptr_t)HS_ATTEND_TOKENS * r->embed_dim, gsize = elem_size(r->grad_dtype);
    HS_TRY(c.disjoint({range("qkv", r->qkv, n * 3 * SE * elem_size(r->qkv_dtype)), range("key_mask", r->key_mask, n * HS_ATTEND_TOKENS),
                       range("grad_out", r->grad_out, n * SE * gsize)},
                      {range("grad_qkv", r->grad_qkv, n * 3 * SE * gsize)}));
    return c.handle_ready(s);
}

// One k_attend_fwd over the rows (the request has passed check_attend).
int launch_attend(hs_sim *, hipStream_t strm, const hs_entity_attend_request *r) {
    hs::AttendArgs a = {};
    a.qkv = r->qkv; a.mask = r->key_mask; a.out = r->out;
    a.n = r->n; a.qkvType = elem_code(r->qkv_dtype); a.outType = elem_code(r->out_dtype);
    const dim3 grid(hs::rows_grid(a.n, hs::kRowsWaves, hs::kRowsMaxGrid)), blk(hs::kRowsThreads);
    with_constant<64, 128>(r->embed_dim, [&](auto e) { hipLaunchKernelGGL((hs::k_attend_fwd<decltype(e)::value>), grid, blk, 0, strm, a); });
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// One k_attend_bwd over the rows (the request has passed check_attend_bwd): no parameters, so no slices and no sum.
int launch_attend_bwd(hs_sim *, hipStream_t strm, const hs_entity_attend_backward_request *r) {
    hs::AttendBwdArgs a = {};
    a.qkv = r->qkv; a.mask = r->key_mask; a.gradOut = r->grad_out; a.gradQkv = r->grad_qkv;
    a.n = r->n; a.qkvType = elem_code(r->qkv_dtype); a.gradType = elem_code(r->grad_dtype);
    const dim3 grid(hs::rows_grid(a.n, hs::kRowsWaves, hs::kRowsMaxGrid)), blk(hs::kRowsThreads);
    with_constant<64, 128>(r->embed_dim, [&](auto e) { hipLaunchKernelGGL((hs::k_attend_bwd<decltype(e)::value>), grid, blk, 0, strm, a); });
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- behaviour statistics (hs_k_behaviour.h) ----
namespace {
static_assert(HS_BEHAVIOUR_STATS == hs::kBehStats && HS_BEHAVIOUR_KIND_STATS == hs::kBehKind && HS_BEHAVIOUR_SIDE_STATS == hs::kBehSide &&
              HS_BEHAVIOUR_UNARMED == hs::kBehUnarmed && HS_BEHAVIOUR_PREP == hs::kBehPrep && HS_BEHAVIOUR_MAIN == hs::kBehMain &&
              HS_BEHAVIOUR_WAITING == hs::kBehWaiting && HS_BEHAVIOUR_WORLD_EPISODES == hs::kBehWorldEpisodes &&
              HS_BEHAVIOUR_REACHED_MAIN == hs::kBehReachedMain && HS_BEHAVIOUR_BAD == hs::kBehBad && HS_BEHAVIOUR_BOXES == hs::kBehBoxes &&
              HS_BEHAVIOUR_RAMPS == hs::kBehRamps && HS_BEHAVIOUR_SEEKERS == hs::kBehSeekers && HS_BEHAVIOUR_HIDERS == hs::kBehHiders &&
              HS_BEHAVIOUR_RAMPS == HS_BEHAVIOUR_BOXES + HS_BEHAVIOUR_KIND_STATS && HS_BEHAVIOUR_SEEKERS == HS_BEHAVIOUR_RAMPS + HS_BEHAVIOUR_KIND_STATS &&
              HS_BEHAVIOUR_HIDERS == HS_BEHAVIOUR_SEEKERS + HS_BEHAVIOUR_SIDE_STATS && HS_BEHAVIOUR_STATS == HS_BEHAVIOUR_HIDERS + HS_BEHAVIOUR_SIDE_STATS,
              "hs_behaviour_request and k_behaviour agree");
static_assert(sizeof(hs_behaviour_request) == 176 && offsetof(hs_behaviour_request, grabbing) == 56 && offsetof(hs_behaviour_request, grab_stride) == 64 &&
              offsetof(hs_behaviour_request, move_eps) == 68 && offsetof(hs_behaviour_request, phase) == 72 && offsetof(hs_behaviour_request, start_pos) == 96 &&
              offsetof(hs_behaviour_request, travel) == 136 && offsetof(hs_behaviour_request, was_active) == 160 && offsetof(hs_behaviour_request, table) == 168,
              "hs_behaviour_request layout (gpu_hideseek/behaviour.py mirrors it)");
static_assert(kExports[HS_EXPORT_GLOBAL_DEBUG_POSITIONS].dtype == HS_DTYPE_F32 && !kExports[HS_EXPORT_GLOBAL_DEBUG_POSITIONS].per_agent &&
              kExports[HS_EXPORT_GLOBAL_DEBUG_POSITIONS].tail[0] == hs::kNumDSlots && kExports[HS_EXPORT_GLOBAL_DEBUG_POSITIONS].tail[1] == 2 &&
              kExports[HS_EXPORT_PREP_COUNTER].dtype == HS_DTYPE_I32 && kExports[HS_EXPORT_PREP_COUNTER].per_agent && kExports[HS_EXPORT_PREP_COUNTER].tail[0] == 1 &&
              kExports[HS_EXPORT_SELF_OBS].dtype == HS_DTYPE_F32 && kExports[HS_EXPORT_SELF_OBS].per_agent && kExports[HS_EXPORT_SELF_OBS].tail[0] == 13 &&
              hs::kMaxBoxes == 9 && hs::kMaxRamps == 2 && hs::kMaxAgents == 6 && hs::kBoxSlot0 == 0 && hs::kRampSlot0 == hs::kMaxBoxes,
              "k_behaviour reads the global_positions, prep_counter and self_data exports and the box and ramp slots");
static_assert(hs::kBehStats * hs::kBehSumSegs <= 1024, "k_behaviour_fold is one workgroup");

// The request with every null input replaced by the handle's own (the state and the table are left as given).
hs::BehaviourArgs behaviour_args(const hs_sim *s, const hs_behaviour_request *r) {
    const hs::SimState &S = s->S;
    return {r->positions ? r->positions : S.xGlobalPos, r->locks, r->counts, r->prep_counter ? r->prep_counter : S.xPrep, r->done ? r->done : S.xDone,
            r->self_type ? r->self_type : S.xSelfType, r->self_mask ? r->self_mask : S.xSelfMask, r->grabbing ? r->grabbing : S.xSelfObs + 12,
            r->grabbing ? r->grab_stride : 13, r->move_eps, S.counts, S.slotOfWorld, S.bmeta, r->phase, r->n_obj, r->n_side, r->start_pos, r->prep_pos,
            r->last_pos, r->prep_locks, r->last_locks, r->travel, r->grab, r->agent_steps, r->was_active, s->behaviour_partials, S.N, s->A};
}

int check_behaviour(hs_sim *s, const hs_behaviour_request *r) {
    const Check c{"hs_behaviour_stats"};
    if (!r) return c.bad("null request");
    if (!r->phase || !r->n_obj || !r->n_side || !r->start_pos || !r->prep_pos || !r->last_pos || !r->prep_locks || !r->last_locks || !r->travel || !r->grab ||
        !r->agent_steps || !r->was_active)
        return c.bad("null state pointer");
    if (!r->table) return c.bad("null table");
    if (!(std::isfinite(r->move_eps) && r->move_eps >= 0.f)) return c.bad("move_eps must be finite and at least 0");
    if (r->grabbing && r->grab_stride < 1) return c.bad("grab_stride must be at least 1 where grabbing is given");
    if (!aligned(4, {r->positions, r->locks, r->counts, r->prep_counter, r->done, r->self_type, r->self_mask, r->grabbing, r->phase, r->n_obj, r->n_side,
                     r->start_pos, r->prep_pos, r->last_pos, r->prep_locks, r->last_locks, r->travel, r->grab, r->agent_steps, r->was_active}))
        return c.bad("every input and state pointer must be 4-byte aligned");
    if (!aligned(8, {r->table})) return c.bad("table must be 8-byte aligned");
    if ((s->S.flags & hs::FLAG_EXT_SKIP_OBSERVATIONS) && (!r->positions || !r->prep_counter || !r->self_type || !r->self_mask || !r->grabbing))
        return c.bad("a null positions, prep_counter, self_type, self_mask or grabbing needs the exports that HS_FLAG_EXT_SKIP_OBSERVATIONS leaves unwritten",
                     HS_ERR_UNSUPPORTED);
    const hs::BehaviourArgs a = behaviour_args(s, r);
    const uintptr_t worlds = (uintptr_t)s->S.N, rows = worlds * (uintptr_t)s->A;
    HS_TRY(c.disjoint({range("positions", a.positions, worlds * 136), range("locks", a.locks, worlds * 44), range("counts", a.counts4, worlds * 16),
                       range("prep_counter", a.prep, rows * 4), range("done", a.done, rows * 4), range("self_type", a.selfType, rows * 4),
                       range("self_mask", a.selfMask, rows * 4), range("grabbing", a.grabbing, ((rows - 1) * (uintptr_t)a.grabStride + 1) * 4)},
                      {range("phase", r->phase, worlds * 4), range("n_obj", r->n_obj, worlds * 8), range("n_side", r->n_side, worlds * 8),
                       range("start_pos", r->start_pos, worlds * 88), range("prep_pos", r->prep_pos, worlds * 88), range("last_pos", r->last_pos, worlds * 136),
                       range("prep_locks", r->prep_locks, worlds * 44), range("last_locks", r->last_locks, worlds * 44), range("travel", r->travel, worlds * 8),
                       range("grab", r->grab, worlds * 8), range("agent_steps", r->agent_steps, worlds * 8), range("was_active", r->was_active, rows * 4),
                       range("table", r->table, HS_BEHAVIOUR_STATS * sizeof(double))}));
    return c.handle_ready(s);
}
// One k_behaviour over every world (the request has passed check_behaviour), then the fixed-order add onto the table.
int launch_behaviour(hs_sim *s, hipStream_t strm, const hs_behaviour_request *r) {
    const hs::BehaviourArgs a = behaviour_args(s, r);
    const int grid = hs::behaviour_grid(a.worlds);
    hipLaunchKernelGGL(hs::k_behaviour<>, dim3(grid), dim3(hs::kBehThreads), 0, strm, a);
    hipLaunchKernelGGL(hs::k_behaviour_fold<>, dim3(1), dim3(hs::kBehStats * hs::kBehSumSegs), 0, strm, (const double *)s->behaviour_partials, grid, r->table);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the dynamic loss scale (hs_k_loss_scale.h) ----
namespace {
static_assert(HS_LOSS_SCALE_STATE == hs::kLossScaleState, "hs_loss_scale and k_adam_step_scaled agree");
static_assert(sizeof(hs_loss_scale) == 48 && offsetof(hs_loss_scale, growth) == 8 && offsetof(hs_loss_scale, min_scale) == 24 &&
              offsetof(hs_loss_scale, growth_interval) == 40 && offsetof(hs_loss_scale, reserved) == 44,
              "hs_loss_scale layout (gpu_hideseek/optim.py mirrors it)");

// x = 2^k exactly, lo <= x <= hi
bool power_of_two_in(double x, double lo, double hi) {
    int k;
    return std::isfinite(x) && x >= lo && x <= hi && std::frexp(x, &k) == 0.5;
}
// The state pointer of a scaled call whose request has passed its own check: the ranges are the request's.
int check_loss_scale_state(const Check &c, const double *state, const std::vector<ByteRange> &ranges) {
    if (!state) return c.bad("null loss_scale_state");
    if (!aligned(8, {state})) return c.bad("loss_scale_state must be 8-byte aligned");
    return c.apart(range("loss_scale_state", state, HS_LOSS_SCALE_STATE * sizeof(double)), ranges);
}
int check_ppo_scaled(hs_sim *s, const hs_ppo_request *r, const double *state) {
    const Check c{"hs_ppo_loss_scaled"};
    HS_TRY(check_ppo(s, r));
    int L;
    size_t nin;
    HS_TRY(c.buckets(r->buckets, &L));
    return check_loss_scale_state(c, state, ppo_ranges(r, L, &nin));
}
int check_twohot_scaled(hs_sim *s, const hs_twohot_request *r, const double *state) {
    const Check c{"hs_twohot_value_scaled"};
    HS_TRY(check_twohot(s, r));
    size_t nin;
    return check_loss_scale_state(c, state, twohot_ranges(r, &nin));
}
int check_adam_scaled(hs_sim *s, const hs_adam_request *r, const hs_loss_scale *ls) {
    const Check c{"hs_adam_step_scaled"};
    HS_TRY(check_adam(s, r));
    if (!ls) return c.bad("null loss scale");
    const double top = std::ldexp(1.0, 126), tiny = std::numeric_limits<double>::denorm_min();
    if (!power_of_two_in(ls->growth, 1.0, top)) return c.bad("growth must be a power of two, at least 1");
    if (!power_of_two_in(ls->backoff, tiny, 1.0)) return c.bad("backoff must be a power of two in (0, 1]");
    if (!power_of_two_in(ls->min_scale, tiny, top) || !power_of_two_in(ls->max_scale, ls->min_scale, top))
        return c.bad("min_scale and max_scale must be powers of two, 0 < min_scale <= max_scale <= 2^126");
    if (ls->growth_interval < 1) return c.bad("growth_interval must be at least 1");
    if (ls->reserved != 0) return c.bad("reserved must be 0");
    return check_loss_scale_state(c, ls->state, adam_ranges(r));
}

// launch_ppo with k_ppo_scaled (the request and the state have passed check_ppo_scaled).
int launch_ppo_scaled(hs_sim *s, hipStream_t strm, const hs_ppo_request *r, const double *state) {
    const hs::PpoArgs a = ppo_args(s, r);
    const dim3 grid(hs::ppo_grid(a.n)), blk(hs::kPpoThreads);
    if (r->mask) hipLaunchKernelGGL(hs::k_ppo_count<>, dim3(a.countParts), blk, 0, strm, r->mask, a.n, s->ppo_counts);
    with_elem(r->logits_dtype, [&](auto tl) {
        with_optional_elem(r->grad_logits, r->grad_dtype, [&](auto tg) {
            with_optional_elem(r->value, r->value_dtype, [&](auto tv) {
                hipLaunchKernelGGL((hs::k_ppo_scaled<decltype(tl), decltype(tg), decltype(tv)>), grid, blk, 0, strm, a, state);
            });
        });
    });
    if (r->stats) launch_partials_sum<double, hs::kPpoStats, hs::kPpoSumSegs>(strm, s->ppo_partials, hs::ppo_grid(a.n), hs::kPpoStats, r->stats);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
// launch_twohot with k_twohot_scaled.
int launch_twohot_scaled(hs_sim *s, hipStream_t strm, const hs_twohot_request *r, const double *state) {
    const hs::TwohotArgs a = twohot_args(s, r);
    const dim3 grid(hs::twohot_grid(a.n)), blk(hs::kTwThreads);
    if (r->mask) hipLaunchKernelGGL(hs::k_ppo_count<>, dim3(a.countParts), dim3(hs::kPpoThreads), 0, strm, r->mask, a.n, s->twohot_counts);
    with_elem(r->logits_dtype, [&](auto tl) {
        with_optional_elem(r->grad_logits, r->grad_dtype, [&](auto tg) {
            with_optional_elem(r->value, r->value_dtype, [&](auto tv) {
                hipLaunchKernelGGL((hs::k_twohot_scaled<decltype(tl), decltype(tg), decltype(tv)>), grid, blk, 0, strm, a, state);
            });
        });
    });
    if (r->stats) launch_partials_sum<double, hs::kTwStats, hs::kTwSumSegs>(strm, s->twohot_partials, hs::twohot_grid(a.n), hs::kTwStats, r->stats);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
// launch_adam with the two scaled kernels: the norm launch also snapshots the loss-scale state, the step launch updates it.
int launch_adam_scaled(hs_sim *s, hipStream_t strm, const hs_adam_request *r, const hs_loss_scale *ls) {
    const hs::AdamArgs a = adam_args(s, r);
    const hs::LossScaleArgs l = {ls->state, ls->growth, ls->backoff, ls->min_scale, ls->max_scale, (double)ls->growth_interval};
    const dim3 blk(hs::kAdamThreads);
    hipLaunchKernelGGL(hs::k_adam_norm_scaled<>, dim3(a.nparts), blk, 0, strm, (const float *)r->grads, a.n, (const double *)r->state,
                       (const double *)ls->state, s->adam_workspace);
    hipLaunchKernelGGL(hs::k_adam_step_scaled<>, dim3(hs::adam_grid(a.n, hs::kAdamStepMaxGrid)), blk, 0, strm, a, l);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the gradient reduction (hs_k_reduce.h) ----
namespace {
static_assert(HS_REDUCE_MAX_SHARDS == hs::kReduceMaxShards, "hs_grad_reduce_request and k_reduce agree");
static_assert(sizeof(hs_grad_reduce_request) == 168 && offsetof(hs_grad_reduce_request, count) == 128 && offsetof(hs_grad_reduce_request, dst) == 136 &&
              offsetof(hs_grad_reduce_request, n) == 144 && offsetof(hs_grad_reduce_request, shards) == 152 && offsetof(hs_grad_reduce_request, total) == 160,
              "hs_grad_reduce_request layout (gpu_hideseek/optim.py mirrors it)");

int check_reduce(hs_sim *s, const hs_grad_reduce_request *r) {
    const Check c{"hs_reduce_gradients"};
    if (!r) return c.bad("null request");
    if (r->shards < 1 || r->shards > HS_REDUCE_MAX_SHARDS) return c.bad("shards must be in [1, HS_REDUCE_MAX_SHARDS]");
    if (r->n < 1 || r->n >= (int64_t)1 << 31) return c.bad("n must be at least 1 and below 2^31");
    if (!r->dst) return c.bad("null dst");
    if (!r->count) return c.bad("null count");
    for (int g = 0; g < r->shards; ++g)
        if (!r->src[g]) return c.bad("null src[" + std::to_string(g) + "]");
    for (int g = 0; g < r->shards; ++g)
        if (!aligned(16, {r->src[g]})) return c.bad("src[" + std::to_string(g) + "] must be 16-byte aligned");
    if (!aligned(16, {r->dst})) return c.bad("dst must be 16-byte aligned");
    if (!aligned(8, {r->count, r->total})) return c.bad("count and total must be 8-byte aligned");
    const uintptr_t bytes = (uintptr_t)r->n * 4;
    const ByteRange dst = range("dst", r->dst, bytes), count = range("count", r->count, (uintptr_t)r->shards * sizeof(double)),
                    total = range("total", r->total, sizeof(double));
    int same = 0;                                                          // dst may be exactly one source, the same address
    for (int g = 0; g < r->shards; ++g) {
        const ByteRange src = range("src", r->src[g], bytes);
        if (r->src[g] == r->dst) ++same;
        else if (overlap(dst, src)) return c.bad("dst overlaps src[" + std::to_string(g) + "] without being it");
        if (overlap(total, src)) return c.bad("total overlaps src[" + std::to_string(g) + "]");
    }
    if (same > 1) return c.bad("dst is more than one of the sources");
    if (overlap(count, dst)) return c.bad("count overlaps dst");
    if (overlap(total, dst)) return c.bad("total overlaps dst");
    if (overlap(total, count)) return c.bad("total overlaps count");
    return c.handle_ready(s);
}

// One k_reduce over the quads (the request has passed check_reduce).  Defined at the end of the file: the kernel is a
// template, emitted where its launch names it, and behind every kernel that was there before it the compiler numbers
// their functions, and with them their branch labels, as before.
int launch_reduce(hs_sim *s, hipStream_t strm, const hs_grad_reduce_request *r);
}  // namespace

// ---- the SimHash encoder (hs_k_hash.h) ----
namespace {
static_assert(HS_HASH_BITS == hs::kHashBits && HS_HASH_BINS == hs::kHashBins && HS_HASH_FEATURES == hs::kHashFeat && HS_HASH_PARAMS == hs::kHashParams &&
              HS_HASH_ROWS_PER_ROUND == hs::kHashRows && HS_HASH_MAX_GRID_BWD == hs::kHashMaxGridBwd && HS_HASH_SUM_SEGS == hs::kRowsSumSegs &&
              HS_HASH_SUM_SEGS == hs::kHashHalves && HS_HASH_SUM_SEGS == HS_EMBED_SUM_SEGS, "hs_hash_encode_request and k_hash agree");
static_assert(sizeof(hs_hash_encode_request) == 48 && offsetof(hs_hash_encode_request, n) == 16 && offsetof(hs_hash_encode_request, features_dtype) == 24 &&
              offsetof(hs_hash_encode_request, eps) == 28 && offsetof(hs_hash_encode_request, features) == 32 && offsetof(hs_hash_encode_request, bin) == 40,
              "hs_hash_encode_request layout (gpu_hideseek/hash_encoder.py mirrors it)");
static_assert(sizeof(hs_hash_encode_backward_request) == 48 && offsetof(hs_hash_encode_backward_request, grad_features) == 8 &&
              offsetof(hs_hash_encode_backward_request, params) == 16 && offsetof(hs_hash_encode_backward_request, n) == 24 &&
              offsetof(hs_hash_encode_backward_request, eps) == 32 && offsetof(hs_hash_encode_backward_request, grad_params) == 40,
              "hs_hash_encode_backward_request layout (gpu_hideseek/hash_encoder.py mirrors it)");

// What the two calls share.
int check_hash_common(const Check &c, const float *params, int32_t n, float eps) {
    if (!params) return c.bad("null params");
    if (!count_ok(n, {HS_PACK_ROW})) return c.bad("n must be at least 1 and n * 296 below 2^31");
    if (!std::isfinite(eps) || !(eps > 0.f)) return c.bad("eps must be finite and > 0");
    return HS_OK;
}

int check_hash(hs_sim *s, const hs_hash_encode_request *r) {
    const Check c{"hs_hash_encode"};
    if (!r) return c.bad("null request");
    if (!r->rows) return c.bad("null rows");
    HS_TRY(check_hash_common(c, r->params, r->n, r->eps));
    if (!r->features) return c.bad("null features");
    HS_TRY(c.dtype(r->rows_dtype, "rows"));
    HS_TRY(c.dtype(r->features_dtype, "features"));
    const uintptr_t rsize = elem_size(r->rows_dtype), fsize = elem_size(r->features_dtype);
    if (!aligned(16, {r->rows})) return c.bad("rows must be 16-byte aligned");
    if (!aligned(4, {r->params})) return c.bad("params must be 4-byte aligned");
    if (!aligned(fsize, {r->features})) return c.bad("features must be aligned to its element size");
    const uintptr_t n = (uintptr_t)r->n;
    HS_TRY(c.disjoint({range("rows", r->rows, n * HS_PACK_ROW * rsize), range("params", r->params, HS_HASH_PARAMS * 4)},
                      {range("features", r->features, n * HS_HASH_FEATURES * fsize), range("bin", r->bin, n)}));
    return c.handle_ready(s);
}

int check_hash_bwd(hs_sim *s, const hs_hash_encode_backward_request *r) {
    const Check c{"hs_hash_encode_backward"};
    if (!r) return c.bad("null request");
    if (!r->bin) return c.bad("null bin");
    if (!r->grad_features) return c.bad("null grad_features");
    HS_TRY(check_hash_common(c, r->params, r->n, r->eps));
    if (!r->grad_params) return c.bad("null grad_params");
    HS_TRY(c.dtype(r->grad_dtype, "grad"));
    const uintptr_t gsize = elem_size(r->grad_dtype);
    if (!aligned(4, {r->params, r->grad_params})) return c.bad("params and grad_params must be 4-byte aligned");
    if (!aligned(gsize, {r->grad_features})) return c.bad("grad_features must be aligned to its element size");
    const uintptr_t n = (uintptr_t)r->n;
    HS_TRY(c.disjoint({range("bin", r->bin, n), range("grad_features", r->grad_features, n * HS_HASH_FEATURES * gsize),
                       range("params", r->params, HS_HASH_PARAMS * 4)},
                      {range("grad_params", r->grad_params, HS_HASH_PARAMS * 4)}));
    return c.handle_ready(s);
}

// Defined at the end of the file, after launch_reduce: the kernels are templates, emitted where their launches name them,
// and behind every kernel that was there before them.
int launch_hash(hs_sim *s, hipStream_t strm, const hs_hash_encode_request *r);
int launch_hash_bwd(hs_sim *s, hipStream_t strm, const hs_hash_encode_backward_request *r);
}  // namespace

namespace {
// Host copy of a tiled column (hs_state.h Col): element (row, world) at ((w / 8) * ROWS + row) * 8 + w % 8.
template <typename T, int ROWS>
struct HostCol {
    std::vector<T> v;
    int load(const hs::Col<T, ROWS> &c, size_t n) {
        v.resize((n + hs::kTile - 1) / hs::kTile * hs::kTile * ROWS);
        HS_HIP(hipMemcpy(v.data(), c.p, v.size() * sizeof(T), hipMemcpyDeviceToHost));
        return HS_OK;
    }
    T operator()(size_t row, size_t p) const { return v[((p >> 3) * ROWS + row) * hs::kTile + (p & 7)]; }     // p = slot
};
int load_slots(hs_sim *s, std::vector<int32_t> &slot) {
    slot.resize(s->S.N);
    HS_HIP(hipMemcpy(slot.data(), s->S.slotOfWorld, slot.size() * 4, hipMemcpyDeviceToHost));
    return HS_OK;
}
}  // namespace

namespace {
// The handle's own stream starts after everything already queued on the device's legacy default stream: that is
// where torch (and scripts/benchmark.py:82-84) writes `action` / `reset` between steps.
int order_after_default_stream(hs_sim *s) {
    HS_HIP(hipEventRecord(s->evIn, nullptr));
    HS_HIP(hipStreamWaitEvent(s->stream, s->evIn, 0));
    return HS_OK;
}
// A blocking call: `launch(s, stream, args...)` on the handle's own stream, after the default stream's work, and waited for.
template <typename... A> int run_blocking(hs_sim *s, int (*launch)(hs_sim *, hipStream_t, A...), std::common_type_t<A>... args) {
    HS_TRY(order_after_default_stream(s));
    HS_TRY(launch(s, s->stream, args...));
    HS_HIP(hipStreamSynchronize(s->stream));
    return HS_OK;
}
// The two forms of a learner entry point: `check(s, args...)`, then `launch` blocking as above, or on the caller's stream.
template <typename... A>
int call_blocking(hs_sim *s, int (*check)(hs_sim *, A...), int (*launch)(hs_sim *, hipStream_t, A...), std::common_type_t<A>... args) {
    HS_ENTER(s, "null sim");
    HS_TRY(check(s, args...));
    return run_blocking(s, launch, args...);
}
template <typename... A>
int call_async(hs_sim *s, void *hip_stream, int (*check)(hs_sim *, A...), int (*launch)(hs_sim *, hipStream_t, A...), std::common_type_t<A>... args) {
    HS_ENTER(s, "null sim");
    HS_TRY(check(s, args...));
    return launch(s, (hipStream_t)hip_stream, args...);
}
}  // namespace

extern "C" {

const char *hs_last_error(void) { return g_err.c_str(); }
const char *hs_version(void) { return "hideseek-mi355x 0.1 (gfx950)"; }

int32_t hs_create(const hs_config *cfg, hs_sim **out) {
    if (!cfg || !out) return fail(HS_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (cfg->exec_mode != HS_EXEC_GPU)
        return fail(HS_ERR_UNSUPPORTED,
                    "exec_mode CPU is not provided by libhideseek: the HIP path is the only execution path");
    const int A = cfg->max_hiders + cfg->max_seekers;
    if (cfg->num_worlds <= 0) return fail(HS_ERR_INVALID_ARG, "num_worlds must be > 0");
    if (A <= 0 || A > hs::kMaxAgents || cfg->max_hiders > 3 || cfg->max_seekers > 3 || cfg->min_hiders < 0 ||
        cfg->min_seekers < 0 || cfg->min_hiders > cfg->max_hiders || cfg->min_seekers > cfg->max_seekers)
        return fail(HS_ERR_INVALID_ARG, "hider/seeker counts out of range (<= 3 each, src/sim.hpp:338-341)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(HS_ERR_NO_DEVICE, "no HIP device visible: libhideseek has no CPU fallback");
    if (cfg->gpu_id < 0 || cfg->gpu_id >= ndev) return fail(HS_ERR_INVALID_ARG, "gpu_id out of range");
    HS_HIP(hipSetDevice(cfg->gpu_id));

    struct Destroy { void operator()(hs_sim *p) const { hs_destroy(p); } };
    std::unique_ptr<hs_sim, Destroy> guard(new hs_sim());      // any return before the release below frees everything
    hs_sim *s = guard.get();
    s->cfg = *cfg;
    s->A = A;
    hs::SimState &S = s->S;
    std::memset(&S, 0, sizeof(S));
    const size_t N = (size_t)cfg->num_worlds, R = N * (size_t)A;
    S.N = (int)N; S.A = A; S.flags = cfg->sim_flags;
    S.initKey = {cfg->rand_seed, 0u};          // rand::initKey (mgr.cpp:678)
    S.minHiders = cfg->min_hiders; S.maxHiders = cfg->max_hiders;
    S.minSeekers = cfg->min_seekers; S.maxSeekers = cfg->max_seekers;
    S.worldOffset = cfg->world_offset;
    const int D = hs::kNumDSlots, AG = hs::kMaxAgents;
#define HS_ALLOC(ptr, ...) HS_TRY(s->dalloc(&(ptr), __VA_ARGS__))
    // tiled columns (hs_state.h Col): whole octets, the padding worlds stay zero = empty slots
    const size_t NP = (N + hs::kTile - 1) / hs::kTile * hs::kTile;
    // the tiled columns are consecutive pieces of ONE arena (so that the periodic deal moves them in one launch): all have
    // 4-byte elements; a column of ROWS rows takes ROWS * NP of them
    {
        const int rows[hs::kBalanceCols] = {S.bpos.kRows, S.brot.kRows, S.blin.kRows, S.bang.kRows, S.bmeta.kRows, S.aforce.kRows, S.walls.kRows,
                                            S.planes.kRows, S.runningScores.kRows, S.grabOther.kRows, S.grabData.kRows};
        s->bal_cols.base[0] = 0;
        for (int k = 0; k < hs::kBalanceCols; ++k) s->bal_cols.base[k + 1] = s->bal_cols.base[k] + rows[k];
        s->col_slots = NP;
        s->col_arena_bytes = (size_t)s->bal_cols.base[hs::kBalanceCols] * NP * 4;
        // (k_observe's staging copy addresses the arena by 32-bit byte offsets from its first column, S.bpos)
        if (s->col_arena_bytes >> 32) return fail(HS_ERR_INVALID_ARG, "hs_create: num_worlds too large, the tiled columns would take 4 GiB or more");
        char *arena, *tmp;
        HS_ALLOC(arena, s->col_arena_bytes); HS_ALLOC(tmp, s->col_arena_bytes);
        s->col_arena = arena; s->bal_tmp = tmp;
        int k = 0;
#define HS_ARENA_COL(col) (col).p = (decltype((col).p))(arena + (size_t)s->bal_cols.base[k++] * NP * 4);
        HS_ARENA_COL(S.bpos) HS_ARENA_COL(S.brot) HS_ARENA_COL(S.blin) HS_ARENA_COL(S.bang) HS_ARENA_COL(S.bmeta) HS_ARENA_COL(S.aforce)
        HS_ARENA_COL(S.walls) HS_ARENA_COL(S.planes) HS_ARENA_COL(S.runningScores) HS_ARENA_COL(S.grabOther) HS_ARENA_COL(S.grabData)
#undef HS_ARENA_COL
    }
    HS_ALLOC(S.numWalls, N); HS_ALLOC(S.numPlanes, N);
    HS_ALLOC(S.curWorldEpisode, N); HS_ALLOC(S.rngKeyA, N); HS_ALLOC(S.rngKeyB, N); HS_ALLOC(S.rngCount, N);
    HS_ALLOC(S.curEpisodeStep, N); HS_ALLOC(S.hiderTeamReward, N); HS_ALLOC(S.counts, N); HS_ALLOC(S.teams, N);
    HS_ALLOC(S.epKeyA, N); HS_ALLOC(S.epKeyB, N);
    // the exported tensors (kExports): descriptor, allocation, and the kernels' pointer to it
    std::memset(s->exports, 0, sizeof(s->exports));
    for (const ExportRow &e : kExports) {
        HS_TRY(alloc_export(s, e.id, e.dtype, {(int64_t)(e.per_agent ? R : N), e.tail[0], e.tail[1]}));
        std::memcpy((char *)&S + e.field, &s->exports[e.id].ptr, sizeof(void *));
    }
    // (every possible pair of every world: 92 KB per world, 1.5 GB at 16 000 worlds, of which a step touches a few MB)
    { char *p; HS_ALLOC(p, NP * hs::kAllDD * sizeof(hs::ManDD)); S.wsDD = p; HS_ALLOC(p, NP * hs::kAllSC * sizeof(hs::ManS)); S.wsSC = p; }
    HS_ALLOC(S.spPair, NP * (hs::kAllDD + hs::kAllSC)); HS_ALLOC(S.spInfo, NP * hs::kSpInfoWords);
    HS_ALLOC(S.phaseTicks, hs::phase_ticks_obs_base((int)N) + 16 * 1024);   // + k_observe's section counters
    HS_ALLOC(S.slotOfWorld, N); HS_ALLOC(S.worldOfSlot, NP); HS_ALLOC(S.loadAcc, N); HS_ALLOC(S.wallHist, N);
    HS_ALLOC(S.slotHdr, NP, 0xFF);                                                          // world id -1: empty slot
    HS_ALLOC(S.lidarSinCos, 60);
    HS_ALLOC(S.octTicks, NP / hs::kTile); HS_ALLOC(S.tickSum, hs::sched_alloc_sums((int)(NP / hs::kTile)));   // + the split schedule's words
    S.stepIdx = hs::step_idx_arg(0, hs::kGroupAll);
    {
        // k_physics holds two waves on each of a CU's four SIMDs.  Two launches place all their waves at once only while
        // some slots stay free: measured at 2 000 octets for 2 048 slots (every wave starts within 12 us) and at 2 048 for
        // 2 048 (a second round of waves, 25 % slower than one chain).  Above 63/64 of the slots a step keeps the one chain.
        int cus = 0;
        HS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->gpu_id));
        const int64_t slots = (int64_t)cus * 4 * 2;
        s->split_fits = (int64_t)(NP / hs::kTile) * 64 <= slots * 63;
    }
    HS_ALLOC(s->bal_hist, hs::kBalanceBins); HS_ALLOC(s->bal_cursor, hs::kBalanceBins); HS_ALLOC(s->bal_new_slot, N);
    HS_ALLOC(S.status, 4);
    if (!(S.flags & hs::FLAG_EXT_SKIP_OBSERVATIONS)) {
        HS_ALLOC(s->pack_partials, (size_t)hs::pack_grid((int)R) * hs::kPackMoments);
        HS_ALLOC(s->pack_routed_partials, std::min<size_t>(hs::kPackMaxGrid, R / hs::kPackRows + hs::kLeagueMaxPolicies) * hs::kPackMoments);   // N G <= both, for every N
    }
    HS_ALLOC(s->gae_partials, (size_t)(hs::gae_grid((int)R) + hs::kLeagueMaxPolicies) * hs::kGaeMoments);      // G gae_grid(R / G) <= that, for every G
    HS_ALLOC(s->ppo_partials, (size_t)hs::kPpoMaxGrid * hs::kPpoStats); HS_ALLOC(s->ppo_counts, hs::kPpoCountGrid);
    HS_ALLOC(s->twohot_partials, (size_t)hs::kTwMaxGrid * hs::kTwStats); HS_ALLOC(s->twohot_counts, hs::kPpoCountGrid);
    HS_ALLOC(s->embed_partials, (size_t)hs::kRowsMaxGridBwd * hs::kEmbParamRows * hs::kEmbMaxE);
    HS_ALLOC(s->lstm_partials, (size_t)hs::kRowsMaxGridBwd * hs::kLstmParamRows * hs::kLstmMaxH);
    HS_ALLOC(s->dense_partials, (size_t)hs::kRowsMaxGridBwd * hs::kDenseParamRows * hs::kDenseMaxC);
    HS_ALLOC(s->hash_partials, (size_t)(hs::kHashMaxGridBwd + 1) * hs::kHashSlice);
    HS_ALLOC(s->adam_workspace, hs::kLossScaleWorkspace);
    HS_ALLOC(s->episode_partials, (size_t)hs::episode_grid((int)N, A) * hs::kEpiStats);
    HS_ALLOC(s->behaviour_partials, (size_t)hs::behaviour_grid((int)N) * hs::kBehStats);
    HS_ALLOC(s->league_step, hs::kLeagueMaxBins + 1);
    HS_ALLOC(s->league_table, hs::kLeagueMaxGroup);
#undef HS_ALLOC
    // Sim::Sim (sim.cpp:1346-1408): resetLevel = 1 for every world, no grab joints
    {
        std::vector<int32_t> ones(N, 1), neg(AG * NP, -1), ident(NP);
        // the first step's groups (ring position 0): every octet early
        const int32_t noct = (int32_t)(NP / hs::kTile);
        std::vector<int32_t> octs(noct);
        for (int32_t i = 0; i < noct; ++i) octs[i] = i;
        if (hipMemcpy(hs::oct_list(S, 0, hs::kGroupEarly, noct), octs.data(), (size_t)noct * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(hs::group_count(S, 0, hs::kGroupEarly), &noct, 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(hs::sched_words(S) + hs::kSchedFactor, &kDefaultLateFactor, 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail(HS_ERR_HIP, "initial upload failed");
        for (size_t i = 0; i < NP; ++i) ident[i] = i < N ? (int32_t)i : -1;      // slot == world until k_balance deals them
        if (hipMemcpy(S.slotOfWorld, ident.data(), N * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(S.worldOfSlot, ident.data(), NP * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(S.xReset, ones.data(), N * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(S.grabOther.p, neg.data(), AG * NP * 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail(HS_ERR_HIP, "initial upload failed");
    }
    for (auto &e : s->ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(HS_ERR_HIP, "hipEventCreate failed");
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&s->evIn, hipEventDisableTiming) != hipSuccess) return fail(HS_ERR_HIP, "stream/event creation failed");
    S.wbeg = 0; S.wcnt = (int)N;
    hipLaunchKernelGGL(hs::k_lidar_table, dim3(1), dim3(64), 0, s->stream, S);
    if (hipStreamSynchronize(s->stream) != hipSuccess) return fail(HS_ERR_HIP, "k_lidar_table failed");
    if ((S.flags & hs::FLAG_EXT_RENDER) && cfg->enable_batch_renderer) {      // rendered by every init / step
        HS_TRY(ensure_render_buffers(s));
    } else {
        s->S.flags &= ~(uint32_t)hs::FLAG_EXT_RENDER;                         // (the flag needs the renderer switched on)
    }
    *out = guard.release();
    return HS_OK;
}

void hs_destroy(hs_sim *s) {
    if (!s) return;
    hipDeviceSynchronize();
    for (void *p : s->allocs) hipFree(p);
    if (s->cams) hipFree(s->cams);
    for (auto &e : s->ev) if (e) hipEventDestroy(e);
    if (s->evIn) hipEventDestroy(s->evIn);
    if (s->stream) hipStreamDestroy(s->stream);
    delete s;
}

int32_t hs_agents_per_world(const hs_sim *s) { return s ? s->A : 0; }

int32_t hs_init(hs_sim *s) {
    HS_ENTER(s, "null sim");
    HS_TRY(run_blocking(s, +[](hs_sim *s, hipStream_t strm) { return launch_step(s, strm, true); }));
    s->initialised = true;
    return HS_OK;
}

namespace {
// A blocking hs_step runs on the device's legacy default stream itself: it is ordered after the caller's writes to
// `action` / `reset` there without a cross-stream event (which costs tens of microseconds per step), and the caller
// waits for it anyway.  hs_step_begin / hs_step_end use the handle's own stream, so that the steps of several handles
// (one per GPU) run side by side.
int step_begin(hs_sim *s, bool own_stream) {
    HS_ENTER(s, "null sim");
    if (s->step_open) return fail(HS_ERR_INVALID_ARG, "hs_step_begin: the previous step was not ended");
    s->step_stream = own_stream ? s->stream : nullptr;
    if (own_stream) HS_TRY(order_after_default_stream(s));
    HS_TRY(launch_step(s, s->step_stream, false, !own_stream));
    s->step_open = true;
    return HS_OK;
}
}  // namespace

int32_t hs_step_begin(hs_sim *s) { return step_begin(s, true); }

int32_t hs_step_end(hs_sim *s) {
    HS_ENTER(s, "null sim");
    if (!s->step_open) return fail(HS_ERR_INVALID_ARG, "hs_step_end without hs_step_begin");
    s->step_open = false;
    if (s->split_open) {                   // the early chain; the late one is on step_stream
        s->split_open = false;
        HS_HIP(hipStreamSynchronize(s->stream));
    }
    HS_HIP(hipStreamSynchronize(s->step_stream));
    if (s->profiling) {
        HS_HIP(hipEventElapsedTime(&s->last_ms[0], s->ev[0], s->ev[1]));
        HS_HIP(hipEventElapsedTime(&s->last_ms[1], s->ev[1], s->ev[2]));
        HS_HIP(hipEventElapsedTime(&s->last_ms[2], s->ev[2], s->ev[3]));
    }
    return poll_status(s);
}

int32_t hs_step(hs_sim *s) {
    HS_TRY(step_begin(s, false));
    return hs_step_end(s);
}

int32_t hs_step_async(hs_sim *s, void *hip_stream) {
    HS_ENTER(s, "null sim");
    HS_TRY(poll_status(s));                // a failure of an earlier asynchronous step surfaces here
    return launch_step(s, (hipStream_t)hip_stream, false);
}

int32_t hs_get_tensor(hs_sim *s, int32_t id, hs_tensor_desc *out) {
    if (!s || !out) return fail(HS_ERR_INVALID_ARG, "null argument");
    if (id < 0 || id >= HS_NUM_EXPORTS) return fail(HS_ERR_INVALID_ARG, "export id out of range");
    if (!s->exports[id].ptr) {
        // renderer outputs are allocated on first request; written only by hs_render / under HS_FLAG_EXT_RENDER
        if (id != HS_EXPORT_RGB && id != HS_EXPORT_DEPTH) return fail(HS_ERR_INVALID_ARG, "export not available");
        HS_HIP(hipSetDevice(s->cfg.gpu_id));
        HS_TRY(ensure_render_buffers(s));
    }
    *out = s->exports[id];
    return HS_OK;
}

int32_t hs_render(hs_sim *s) {
    HS_ENTER(s, "null sim");
    if (!s->initialised) return fail(HS_ERR_INVALID_ARG, "hs_render before hs_init");
    if (s->step_open) return fail(HS_ERR_INVALID_ARG, "hs_render inside an open step");
    HS_TRY(ensure_render_buffers(s));
    return run_blocking(s, +[](hs_sim *s, hipStream_t strm) -> int {
        launch_render(s, strm);
        HS_HIP(hipGetLastError());
        return HS_OK;
    });
}

static_assert(sizeof(hs_camera) == sizeof(hs::SpectateCam) && offsetof(hs_camera, rot) == offsetof(hs::SpectateCam, rot) &&
              offsetof(hs_camera, tan_half_fov_y) == offsetof(hs::SpectateCam, tanHalfFovY), "hs_camera layout");
static_assert((int)HS_SPECTATE_NO_CULL == (int)hs::kSpectateNoCull, "HS_SPECTATE_NO_CULL");

int32_t hs_render_cameras(hs_sim *s, const hs_camera *cams, int32_t n, int32_t W, int32_t H, uint32_t flags, float *depth,
                          uint8_t *rgba, int32_t *hit) {
    HS_ENTER(s, "null sim");
    if (!s->initialised) return fail(HS_ERR_INVALID_ARG, "hs_render_cameras before hs_init");
    if (s->step_open) return fail(HS_ERR_INVALID_ARG, "hs_render_cameras inside an open step");
    if (!cams || n < 1) return fail(HS_ERR_INVALID_ARG, "hs_render_cameras: need at least one camera");
    if (W < 1 || W > 4096 || H < 1 || H > 4096) return fail(HS_ERR_INVALID_ARG, "hs_render_cameras: width / height outside [1, 4096]");
    if (flags & ~(uint32_t)HS_SPECTATE_NO_CULL) return fail(HS_ERR_INVALID_ARG, "hs_render_cameras: unknown flags");
    if (!depth && !rgba && !hit) return fail(HS_ERR_INVALID_ARG, "hs_render_cameras: every output is null");
    if (((uintptr_t)depth | (uintptr_t)rgba | (uintptr_t)hit) & 3u) return fail(HS_ERR_INVALID_ARG, "hs_render_cameras: outputs must be 4-byte aligned");
    for (int32_t i = 0; i < n; ++i) {
        const hs_camera &c = cams[i];
        auto at = [i] { return "hs_render_cameras: camera " + std::to_string(i) + ": "; };
        if (c.world < 0 || c.world >= s->S.N) return fail(HS_ERR_INVALID_ARG, at() + "world index out of range");
        bool finite = std::isfinite(c.tan_half_fov_y);
        for (float v : c.pos) finite = finite && std::isfinite(v);
        for (float v : c.rot) finite = finite && std::isfinite(v);
        if (!finite) return fail(HS_ERR_INVALID_ARG, at() + "non-finite pose or field of view");
        const double q2 = (double)c.rot[0] * c.rot[0] + (double)c.rot[1] * c.rot[1] + (double)c.rot[2] * c.rot[2] + (double)c.rot[3] * c.rot[3];
        if (!(q2 >= 0.99 && q2 <= 1.01)) return fail(HS_ERR_INVALID_ARG, at() + "rotation is not a unit quaternion (|q|^2 outside [0.99, 1.01])");
        if (!(c.tan_half_fov_y > 0.f)) return fail(HS_ERR_INVALID_ARG, at() + "tan_half_fov_y must be > 0");
    }
    if (n > s->cam_cap) {
        if (s->cams) { HS_HIP(hipStreamSynchronize(s->stream)); HS_HIP(hipFree(s->cams)); s->cams = nullptr; s->cam_cap = 0; }
        HS_HIP(hipMalloc(&s->cams, (size_t)n * sizeof(hs::SpectateCam)));
        s->cam_cap = n;
    }
    HS_TRY(order_after_default_stream(s));
    HS_HIP(hipMemcpyAsync(s->cams, cams, (size_t)n * sizeof(hs_camera), hipMemcpyHostToDevice, s->stream));
    const int tilesX = (W + hs::kSpectateTileW - 1) / hs::kSpectateTileW, tilesY = (H + hs::kSpectateTileH - 1) / hs::kSpectateTileH;
    const int tilesPerCam = tilesX * tilesY;
    const int perLaunch = std::max(1, (1 << 22) / tilesPerCam);      // cameras per launch: the grid stays far below 2^32 threads
    for (int c0 = 0; c0 < n; c0 += perLaunch) {
        const int nc = std::min(perLaunch, n - c0);
        hipLaunchKernelGGL(hs::k_spectate, dim3((unsigned)(nc * tilesPerCam)), dim3(hs::kSpectateThreads), 0, s->stream, s->S,
                           (const hs::SpectateCam *)s->cams, c0, (int)W, (int)H, tilesX, tilesPerCam, (unsigned)flags, depth,
                           (unsigned *)rgba, (int *)hit);
    }
    HS_HIP(hipGetLastError());
    HS_HIP(hipStreamSynchronize(s->stream));
    return HS_OK;
}

int32_t hs_trigger_reset(hs_sim *s, int32_t world, int32_t level) {
    HS_ENTER(s && world >= 0 && world < s->S.N, "world index out of range");
    HS_HIP(hipMemcpy(s->S.xReset + world, &level, sizeof(int32_t), hipMemcpyHostToDevice));
    return HS_OK;
}

int32_t hs_set_action(hs_sim *s, int32_t agent, int32_t x, int32_t y, int32_t r, int32_t g, int32_t l) {
    HS_ENTER(s && agent >= 0 && agent < s->S.N * s->A, "agent index out of range");
    int32_t a[5] = {x, y, r, g ? 1 : 0, l ? 1 : 0};
    HS_HIP(hipMemcpy(s->S.xAction + (size_t)agent * 5, a, sizeof(a), hipMemcpyHostToDevice));
    return HS_OK;
}

// ---- checkpoints (sim.cpp:956-1137, 1315-1333) ----
namespace {
int launch_save_ckpts(hs_sim *s, hipStream_t strm) {
    hipLaunchKernelGGL(hs::k_save_ckpt, dim3((s->S.N + 63) / 64), dim3(64), 0, strm, s->S);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
int launch_load_ckpts(hs_sim *s, hipStream_t strm) {
    hipLaunchKernelGGL(hs::k_load_ckpt, dim3((s->S.N + 63) / 64), dim3(64), 0, strm, s->S);
    launch_observe(s, strm);              // postGenTasks + observationsTasks for every world (sim.cpp:1331-1332)
    HS_HIP(hipGetLastError());
    return HS_OK;
}
int set_ckpt_trigger(hs_sim *s, int32_t world) {
    if (world < 0 || world >= s->S.N) return fail(HS_ERR_INVALID_ARG, "world index out of range");
    const int32_t one = 1;
    HS_HIP(hipMemcpy(s->S.xCkptCtrl + world, &one, sizeof(one), hipMemcpyHostToDevice));
    return HS_OK;
}
}  // namespace

int32_t hs_save_checkpoints(hs_sim *s) {
    HS_ENTER(s, "null sim");
    return run_blocking(s, launch_save_ckpts);
}
int32_t hs_load_checkpoints(hs_sim *s) {
    HS_ENTER(s, "null sim");
    return run_blocking(s, launch_load_ckpts);
}
int32_t hs_save_checkpoint(hs_sim *s, int32_t world) {
    HS_ENTER(s, "null sim");
    HS_TRY(set_ckpt_trigger(s, world));
    return run_blocking(s, launch_save_ckpts);
}
int32_t hs_load_checkpoint(hs_sim *s, int32_t world) {
    HS_ENTER(s, "null sim");
    HS_TRY(set_ckpt_trigger(s, world));
    return run_blocking(s, launch_load_ckpts);
}

// ---- stream entry points with the reference's JAX buffer order (mgr.cpp:168-201, 362-436) ----
namespace {
int copy_dd(void *dst, const void *src, size_t bytes, hipStream_t strm) {
    if (!dst || !src) return fail(HS_ERR_INVALID_ARG, "null device buffer");
    if (dst == src) return HS_OK;                // the caller passed the simulator's own tensor
    HS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, strm));
    return HS_OK;
}
// One operand or result of a stream entry point: the caller's buffer into / out of export `id`, all of its bytes.
int copy_in(hs_sim *s, int id, const void *src, hipStream_t strm) { return copy_dd(s->exports[id].ptr, src, bytes_of(s, id), strm); }
int copy_out(hs_sim *s, int id, void *dst, hipStream_t strm) { return copy_dd(dst, s->exports[id].ptr, bytes_of(s, id), strm); }

// Manager::trainInterface (mgr.cpp:1338-1375), in its order (hs_train_interface)
const hs_iface_entry kTrainInterface[] = {
    {"actions", HS_ROLE_ACTION, HS_EXPORT_ACTION},
    {"resets", HS_ROLE_RESET, HS_EXPORT_RESET},
    {"sim_ctrl", HS_ROLE_SIM_CTRL, -1},
    {"policy_assignments", HS_ROLE_PBT_INPUT, HS_EXPORT_AGENT_POLICY},
    {"prep_counter", HS_ROLE_OBSERVATION, HS_EXPORT_PREP_COUNTER},
    {"self_data", HS_ROLE_OBSERVATION, HS_EXPORT_SELF_OBS},
    {"self_type", HS_ROLE_OBSERVATION, HS_EXPORT_SELF_TYPE},
    {"self_mask", HS_ROLE_OBSERVATION, HS_EXPORT_SELF_MASK},
    {"self_lidar", HS_ROLE_OBSERVATION, HS_EXPORT_LIDAR},
    {"agent_data", HS_ROLE_OBSERVATION, HS_EXPORT_AGENT_OBS},
    {"box_data", HS_ROLE_OBSERVATION, HS_EXPORT_BOX_OBS},
    {"ramp_data", HS_ROLE_OBSERVATION, HS_EXPORT_RAMP_OBS},
    {"vis_agents_mask", HS_ROLE_OBSERVATION, HS_EXPORT_AGENT_VIS_MASKS},
    {"vis_boxes_mask", HS_ROLE_OBSERVATION, HS_EXPORT_BOX_VIS_MASKS},
    {"vis_ramps_mask", HS_ROLE_OBSERVATION, HS_EXPORT_RAMP_VIS_MASKS},
    {"rewards", HS_ROLE_REWARD, HS_EXPORT_REWARD},
    {"dones", HS_ROLE_DONE, HS_EXPORT_DONE},
    {"episode_results", HS_ROLE_PBT_OUTPUT, HS_EXPORT_EPISODE_RESULT},
    {"checkpoint_data", HS_ROLE_CHECKPOINT, HS_EXPORT_CHECKPOINT},
};
// copyOutObservations (mgr.cpp:340-360): the observation rows of the interface, in its order; returns the advanced
// buffer cursor through *pp
int copy_out_observations(hs_sim *s, hipStream_t strm, void ***pp) {
    for (const hs_iface_entry &e : kTrainInterface)
        if (e.role == HS_ROLE_OBSERVATION) HS_TRY(copy_out(s, e.export_id, *(*pp)++, strm));
    return HS_OK;
}
}  // namespace

int32_t hs_jax_init(hs_sim *s, void *hip_stream, void **buffers) {
    HS_ENTER(s && buffers, "null argument");
    hipStream_t strm = (hipStream_t)hip_stream;
    HS_TRY(launch_step(s, strm, true));
    HS_TRY(copy_out_observations(s, strm, &buffers));
    HS_HIP(hipStreamSynchronize(strm));          // gpuStreamInit synchronises (mgr.cpp:376)
    s->initialised = true;
    return HS_OK;
}
int32_t hs_jax_step(hs_sim *s, void *hip_stream, void **buffers) {
    HS_ENTER(s && buffers, "null argument");
    hipStream_t strm = (hipStream_t)hip_stream;
    HS_TRY(poll_status(s));                // a failure of an earlier asynchronous step surfaces here
    HS_TRY(copy_in(s, HS_EXPORT_ACTION, *buffers++, strm));
    HS_TRY(copy_in(s, HS_EXPORT_RESET, *buffers++, strm));
    HS_TRY(copy_in(s, HS_EXPORT_AGENT_POLICY, *buffers++, strm));
    HS_TRY(launch_step(s, strm, false));
    HS_TRY(copy_out_observations(s, strm, &buffers));
    HS_TRY(copy_out(s, HS_EXPORT_REWARD, *buffers++, strm));
    HS_TRY(copy_out(s, HS_EXPORT_DONE, *buffers++, strm));
    return copy_out(s, HS_EXPORT_EPISODE_RESULT, *buffers++, strm);
}
int32_t hs_jax_save_checkpoints(hs_sim *s, void *hip_stream, void **buffers) {
    HS_ENTER(s && buffers, "null argument");
    hipStream_t strm = (hipStream_t)hip_stream;
    HS_TRY(copy_in(s, HS_EXPORT_CHECKPOINT_CONTROL, buffers[0], strm));
    HS_TRY(launch_save_ckpts(s, strm));
    return copy_out(s, HS_EXPORT_CHECKPOINT, buffers[1], strm);
}
int32_t hs_jax_load_checkpoints(hs_sim *s, void *hip_stream, void **buffers) {
    HS_ENTER(s && buffers, "null argument");
    hipStream_t strm = (hipStream_t)hip_stream;
    HS_TRY(copy_in(s, HS_EXPORT_CHECKPOINT_CONTROL, *buffers++, strm));
    HS_TRY(copy_in(s, HS_EXPORT_CHECKPOINT, *buffers++, strm));
    HS_TRY(launch_load_ckpts(s, strm));
    return copy_out_observations(s, strm, &buffers);
}

// ---- the learner calls (check_* / launch_* above) ----
int32_t hs_pack_policy_inputs(hs_sim *s, const hs_pack_request *req) { return call_blocking(s, check_pack, launch_pack, req); }
int32_t hs_pack_policy_inputs_async(hs_sim *s, void *hip_stream, const hs_pack_request *req) { return call_async(s, hip_stream, check_pack, launch_pack, req); }
int32_t hs_sample_actions(hs_sim *s, const hs_sample_request *req) { return call_blocking(s, check_sample, launch_sample, req); }
int32_t hs_sample_actions_async(hs_sim *s, void *hip_stream, const hs_sample_request *req) { return call_async(s, hip_stream, check_sample, launch_sample, req); }
int32_t hs_compute_gae(hs_sim *s, const hs_gae_request *req) { return call_blocking(s, check_gae, launch_gae, req); }
int32_t hs_compute_gae_async(hs_sim *s, void *hip_stream, const hs_gae_request *req) { return call_async(s, hip_stream, check_gae, launch_gae, req); }
int32_t hs_ppo_loss(hs_sim *s, const hs_ppo_request *req) { return call_blocking(s, check_ppo, launch_ppo, req); }
int32_t hs_ppo_loss_async(hs_sim *s, void *hip_stream, const hs_ppo_request *req) { return call_async(s, hip_stream, check_ppo, launch_ppo, req); }
int32_t hs_twohot_value(hs_sim *s, const hs_twohot_request *req) { return call_blocking(s, check_twohot, launch_twohot, req); }
int32_t hs_twohot_value_async(hs_sim *s, void *hip_stream, const hs_twohot_request *req) { return call_async(s, hip_stream, check_twohot, launch_twohot, req); }
int32_t hs_ppo_loss_scaled(hs_sim *s, const hs_ppo_request *req, const double *loss_scale_state) {
    return call_blocking(s, check_ppo_scaled, launch_ppo_scaled, req, loss_scale_state);
}
int32_t hs_ppo_loss_scaled_async(hs_sim *s, void *hip_stream, const hs_ppo_request *req, const double *loss_scale_state) {
    return call_async(s, hip_stream, check_ppo_scaled, launch_ppo_scaled, req, loss_scale_state);
}
int32_t hs_twohot_value_scaled(hs_sim *s, const hs_twohot_request *req, const double *loss_scale_state) {
    return call_blocking(s, check_twohot_scaled, launch_twohot_scaled, req, loss_scale_state);
}
int32_t hs_twohot_value_scaled_async(hs_sim *s, void *hip_stream, const hs_twohot_request *req, const double *loss_scale_state) {
    return call_async(s, hip_stream, check_twohot_scaled, launch_twohot_scaled, req, loss_scale_state);
}
int32_t hs_entity_encode(hs_sim *s, const hs_entity_encode_request *req) { return call_blocking(s, check_embed, launch_embed, req); }
int32_t hs_entity_encode_async(hs_sim *s, void *hip_stream, const hs_entity_encode_request *req) { return call_async(s, hip_stream, check_embed, launch_embed, req); }
int32_t hs_entity_encode_backward(hs_sim *s, const hs_entity_encode_backward_request *req) { return call_blocking(s, check_embed_bwd, launch_embed_bwd, req); }
int32_t hs_entity_encode_backward_async(hs_sim *s, void *hip_stream, const hs_entity_encode_backward_request *req) { return call_async(s, hip_stream, check_embed_bwd, launch_embed_bwd, req); }
int32_t hs_lstm_cell(hs_sim *s, const hs_lstm_cell_request *req) { return call_blocking(s, check_lstm, launch_lstm, req); }
int32_t hs_lstm_cell_async(hs_sim *s, void *hip_stream, const hs_lstm_cell_request *req) { return call_async(s, hip_stream, check_lstm, launch_lstm, req); }
int32_t hs_lstm_cell_backward(hs_sim *s, const hs_lstm_cell_backward_request *req) { return call_blocking(s, check_lstm_bwd, launch_lstm_bwd, req); }
int32_t hs_lstm_cell_backward_async(hs_sim *s, void *hip_stream, const hs_lstm_cell_backward_request *req) { return call_async(s, hip_stream, check_lstm_bwd, launch_lstm_bwd, req); }
int32_t hs_dense_norm_act(hs_sim *s, const hs_dense_norm_act_request *req) { return call_blocking(s, check_dense, launch_dense, req); }
int32_t hs_dense_norm_act_async(hs_sim *s, void *hip_stream, const hs_dense_norm_act_request *req) { return call_async(s, hip_stream, check_dense, launch_dense, req); }
int32_t hs_dense_norm_act_backward(hs_sim *s, const hs_dense_norm_act_backward_request *req) { return call_blocking(s, check_dense_bwd, launch_dense_bwd, req); }
int32_t hs_dense_norm_act_backward_async(hs_sim *s, void *hip_stream, const hs_dense_norm_act_backward_request *req) { return call_async(s, hip_stream, check_dense_bwd, launch_dense_bwd, req); }
int32_t hs_adam_step(hs_sim *s, const hs_adam_request *req) { return call_blocking(s, check_adam, launch_adam, req); }
int32_t hs_adam_step_async(hs_sim *s, void *hip_stream, const hs_adam_request *req) { return call_async(s, hip_stream, check_adam, launch_adam, req); }
int32_t hs_adam_step_scaled(hs_sim *s, const hs_adam_request *req, const hs_loss_scale *ls) {
    return call_blocking(s, check_adam_scaled, launch_adam_scaled, req, ls);
}
int32_t hs_adam_step_scaled_async(hs_sim *s, void *hip_stream, const hs_adam_request *req, const hs_loss_scale *ls) {
    return call_async(s, hip_stream, check_adam_scaled, launch_adam_scaled, req, ls);
}
int32_t hs_reduce_gradients(hs_sim *s, const hs_grad_reduce_request *req) { return call_blocking(s, check_reduce, launch_reduce, req); }
int32_t hs_reduce_gradients_async(hs_sim *s, void *hip_stream, const hs_grad_reduce_request *req) {
    return call_async(s, hip_stream, check_reduce, launch_reduce, req);
}
int32_t hs_gather_sequences(hs_sim *s, const hs_gather_request *req) { return call_blocking(s, check_gather, launch_gather, req); }
int32_t hs_gather_sequences_async(hs_sim *s, void *hip_stream, const hs_gather_request *req) { return call_async(s, hip_stream, check_gather, launch_gather, req); }
int32_t hs_episode_stats(hs_sim *s, const hs_episode_request *req) { return call_blocking(s, check_episode, launch_episode, req); }
int32_t hs_episode_stats_async(hs_sim *s, void *hip_stream, const hs_episode_request *req) { return call_async(s, hip_stream, check_episode, launch_episode, req); }
int32_t hs_behaviour_stats(hs_sim *s, const hs_behaviour_request *req) { return call_blocking(s, check_behaviour, launch_behaviour, req); }
int32_t hs_behaviour_stats_async(hs_sim *s, void *hip_stream, const hs_behaviour_request *req) {
    return call_async(s, hip_stream, check_behaviour, launch_behaviour, req);
}
int32_t hs_league_step(hs_sim *s, const hs_league_request *req) { return call_blocking(s, check_league, launch_league, req); }
int32_t hs_league_step_async(hs_sim *s, void *hip_stream, const hs_league_request *req) { return call_async(s, hip_stream, check_league, launch_league, req); }
int32_t hs_league_set_schedule(hs_sim *s, const int32_t *pairs_host, int32_t group, int32_t num_policies) {
    HS_ENTER(s, "null sim");
    return set_league_schedule(s, pairs_host, group, num_policies);
}
int32_t hs_league_step_scheduled(hs_sim *s, const hs_league_request *req) { return call_blocking(s, check_league_scheduled, launch_league_scheduled, req); }
int32_t hs_league_step_scheduled_async(hs_sim *s, void *hip_stream, const hs_league_request *req) {
    return call_async(s, hip_stream, check_league_scheduled, launch_league_scheduled, req);
}
int32_t hs_pack_policy_inputs_routed(hs_sim *s, const hs_pack_routed_request *req) { return call_blocking(s, check_pack_routed, launch_pack_routed, req); }
int32_t hs_pack_policy_inputs_routed_async(hs_sim *s, void *hip_stream, const hs_pack_routed_request *req) { return call_async(s, hip_stream, check_pack_routed, launch_pack_routed, req); }
int32_t hs_sample_actions_routed(hs_sim *s, const hs_sample_routed_request *req) { return call_blocking(s, check_sample_routed, launch_sample_routed, req); }
int32_t hs_sample_actions_routed_async(hs_sim *s, void *hip_stream, const hs_sample_routed_request *req) { return call_async(s, hip_stream, check_sample_routed, launch_sample_routed, req); }
int32_t hs_compute_gae_grouped(hs_sim *s, const hs_gae_grouped_request *req) { return call_blocking(s, check_gae_grouped, launch_gae_grouped, req); }
int32_t hs_compute_gae_grouped_async(hs_sim *s, void *hip_stream, const hs_gae_grouped_request *req) { return call_async(s, hip_stream, check_gae_grouped, launch_gae_grouped, req); }
int32_t hs_entity_attend(hs_sim *s, const hs_entity_attend_request *req) { return call_blocking(s, check_attend, launch_attend, req); }
int32_t hs_entity_attend_async(hs_sim *s, void *hip_stream, const hs_entity_attend_request *req) { return call_async(s, hip_stream, check_attend, launch_attend, req); }
int32_t hs_entity_attend_backward(hs_sim *s, const hs_entity_attend_backward_request *req) { return call_blocking(s, check_attend_bwd, launch_attend_bwd, req); }
int32_t hs_entity_attend_backward_async(hs_sim *s, void *hip_stream, const hs_entity_attend_backward_request *req) { return call_async(s, hip_stream, check_attend_bwd, launch_attend_bwd, req); }
int32_t hs_hash_encode(hs_sim *s, const hs_hash_encode_request *req) { return call_blocking(s, check_hash, launch_hash, req); }
int32_t hs_hash_encode_async(hs_sim *s, void *hip_stream, const hs_hash_encode_request *req) { return call_async(s, hip_stream, check_hash, launch_hash, req); }
int32_t hs_hash_encode_backward(hs_sim *s, const hs_hash_encode_backward_request *req) { return call_blocking(s, check_hash_bwd, launch_hash_bwd, req); }
int32_t hs_hash_encode_backward_async(hs_sim *s, void *hip_stream, const hs_hash_encode_backward_request *req) {
    return call_async(s, hip_stream, check_hash_bwd, launch_hash_bwd, req);
}
int32_t hs_obs_norm_update(hs_sim *s, const hs_obs_norm_request *req) { return call_blocking(s, check_norm_update, launch_norm_update, req); }
int32_t hs_obs_norm_update_async(hs_sim *s, void *hip_stream, const hs_obs_norm_request *req) { return call_async(s, hip_stream, check_norm_update, launch_norm_update, req); }
int32_t hs_pack_policy_inputs_normalized(hs_sim *s, const hs_pack_request *req, const float *table) {
    return call_blocking(s, check_pack_norm, launch_pack_norm, req, table);
}
int32_t hs_pack_policy_inputs_normalized_async(hs_sim *s, void *hip_stream, const hs_pack_request *req, const float *table) {
    return call_async(s, hip_stream, check_pack_norm, launch_pack_norm, req, table);
}

// ---- XLA custom-call targets (the original, status-less GPU custom-call ABI) ----
// What madrona::py::JAXInterface registers with XLA for the four Manager functions above (src/bindings.cpp:97-118):
// XLA calls target(stream, buffers, opaque, opaque_len) from its own stream-executor thread; `opaque` is the
// descriptor the Python side attached to the call — here the 8 bytes of the simulator handle.  The ABI has no status
// channel: a failure is kept (hs_xla_last_status, hs_last_error on the calling thread is not the user's thread) and
// surfaces as HS_ERR_HIP from the next blocking call on the handle, like a failed asynchronous step.
namespace {
std::atomic<int32_t> g_xla_status{HS_OK};
void xla_call(int32_t (*FN)(hs_sim *, void *, void **), void *stream, void **buffers, const char *opaque, size_t opaque_len) {
    hs_sim *s = nullptr;
    if (opaque && opaque_len == sizeof(s)) memcpy(&s, opaque, sizeof(s));
    const int32_t rc = s ? FN(s, stream, buffers) : (int32_t)HS_ERR_INVALID_ARG;
    if (rc != HS_OK) { g_xla_status.store(rc); if (s) s->async_error.store(rc); }
}
}  // namespace
void hs_xla_init(void *stream, void **buffers, const char *opaque, size_t opaque_len) { xla_call(hs_jax_init, stream, buffers, opaque, opaque_len); }
void hs_xla_step(void *stream, void **buffers, const char *opaque, size_t opaque_len) { xla_call(hs_jax_step, stream, buffers, opaque, opaque_len); }
void hs_xla_save_checkpoints(void *stream, void **buffers, const char *opaque, size_t opaque_len) { xla_call(hs_jax_save_checkpoints, stream, buffers, opaque, opaque_len); }
void hs_xla_load_checkpoints(void *stream, void **buffers, const char *opaque, size_t opaque_len) { xla_call(hs_jax_load_checkpoints, stream, buffers, opaque, opaque_len); }
int32_t hs_xla_last_status(int32_t clear) { return clear ? g_xla_status.exchange(HS_OK) : g_xla_status.load(); }

// Development aid (HS_PHASE_TIMING builds): accumulated wall-clock ticks per phase per workgroup of k_physics.
int32_t hs_debug_phase_ticks(hs_sim *s, int64_t *out, int32_t max_groups) {
    HS_ENTER(s && out, "null argument");
    int nb = (s->S.N + hs::kTile - 1) / hs::kTile;          // one workgroup (wave) per octet
    if (nb > max_groups) nb = max_groups;
    HS_HIP(hipMemcpy(out, s->S.phaseTicks, (size_t)nb * 10 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return nb;
}

// The same for k_observe: ticks per section summed over all waves (HS_PHASE_TIMING builds).
int32_t hs_debug_observe_ticks(hs_sim *s, int64_t out[16]) {
    HS_ENTER(s && out, "null argument");
    std::vector<int64_t> part(16 * 1024);
    HS_HIP(hipMemcpy(part.data(), s->S.phaseTicks + hs::phase_ticks_obs_base(s->S.N), part.size() * sizeof(int64_t),
                     hipMemcpyDeviceToHost));
    for (int i = 0; i < 16; ++i) { out[i] = 0; for (int b = 0; b < 1024; ++b) out[i] += part[(size_t)b * 16 + i]; }
    return HS_OK;
}

int32_t hs_debug_dump_bodies(hs_sim *s, float *bodies, int32_t *meta) {
    HS_ENTER(s && bodies && meta, "null argument");
    HS_HIP(hipDeviceSynchronize());
    const size_t N = s->S.N, D = hs::kNumDSlots;
    HostCol<float, 3 * hs::kNumDSlots> pos, lin, ang; HostCol<float, 4 * hs::kNumDSlots> rot; HostCol<int, hs::kNumDSlots> m;
    int rc;
    if ((rc = pos.load(s->S.bpos, N)) != HS_OK || (rc = rot.load(s->S.brot, N)) != HS_OK || (rc = lin.load(s->S.blin, N)) != HS_OK ||
        (rc = ang.load(s->S.bang, N)) != HS_OK || (rc = m.load(s->S.bmeta, N)) != HS_OK) return rc;
    std::vector<int32_t> slot;
    if ((rc = load_slots(s, slot)) != HS_OK) return rc;
    for (size_t w = 0; w < N; ++w)
        for (size_t i = 0; i < D; ++i) {
            const size_t p = (size_t)slot[w];
            float *o = bodies + (w * D + i) * 13;
            for (size_t c = 0; c < 3; ++c) { o[c] = pos(c * D + i, p); o[7 + c] = lin(c * D + i, p); o[10 + c] = ang(c * D + i, p); }
            for (size_t c = 0; c < 4; ++c) o[3 + c] = rot(c * D + i, p);
            int32_t mm = m(i, p);
            int32_t *om = meta + (w * D + i) * 3;
            if (mm == 0) { om[0] = -1; om[1] = 2; om[2] = 0; }
            else { om[0] = (mm & 0xff) - 1; om[1] = (mm >> 8) & 0xff; om[2] = (mm >> 16) & 0xff; }
        }
    return HS_OK;
}

int32_t hs_debug_dump_walls(hs_sim *s, float *walls, int32_t *info) {
    HS_ENTER(s && walls && info, "null argument");
    HS_HIP(hipDeviceSynchronize());
    const size_t N = s->S.N, K = hs::kMaxWalls;
    HostCol<float, 4 * hs::kMaxWalls> wl;
    int rc;
    if ((rc = wl.load(s->S.walls, N)) != HS_OK) return rc;
    std::vector<int32_t> nw(N), np(N), cnt(N), step(N);
    HS_HIP(hipMemcpy(nw.data(), s->S.numWalls, N * 4, hipMemcpyDeviceToHost));
    HS_HIP(hipMemcpy(np.data(), s->S.numPlanes, N * 4, hipMemcpyDeviceToHost));
    HS_HIP(hipMemcpy(cnt.data(), s->S.counts, N * 4, hipMemcpyDeviceToHost));
    HS_HIP(hipMemcpy(step.data(), s->S.curEpisodeStep, N * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> slot;
    if ((rc = load_slots(s, slot)) != HS_OK) return rc;
    for (size_t w = 0; w < N; ++w) {
        for (size_t k = 0; k < K; ++k)
            for (size_t c = 0; c < 4; ++c)
                walls[(w * K + k) * 4 + c] = (int)k < nw[w] ? wl(c * K + k, (size_t)slot[w]) : 0.f;
        int32_t *m = info + w * 8;
        const int c = cnt[w];
        m[0] = nw[w]; m[1] = np[w]; m[2] = (c >> 12) & 15; m[3] = (c >> 16) & 15; m[4] = c & 15; m[5] = (c >> 4) & 15;
        m[6] = step[w]; m[7] = (c >> 20) & 1;
    }
    return HS_OK;
}

// PMC calibration (MI355X_MICROARCH.md: FETCH_SIZE is uncalibrated for narrow accesses): copies `bytes`
// with the access pattern of the simulator's SoA columns — one coalesced dword per lane.
__global__ void k_calib_copy_dword(const float *in, float *out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = in[i] + 1.f;
}
int32_t hs_debug_calibrate(int64_t bytes) {
    if (bytes <= 0) return fail(HS_ERR_INVALID_ARG, "bytes must be > 0");
    float *a = nullptr, *b = nullptr;
    HS_HIP(hipMalloc((void **)&a, (size_t)bytes));
    HS_HIP(hipMalloc((void **)&b, (size_t)bytes));
    HS_HIP(hipMemset(a, 0, (size_t)bytes));
    hipLaunchKernelGGL(k_calib_copy_dword, dim3(4096), dim3(256), 0, nullptr, a, b, (size_t)bytes / 4);
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipFree(a)); HS_HIP(hipFree(b));
    return HS_OK;
}

// hs_debug_dump_hull: the hull tables as the kernels see them (hs_collide.h), one lane.
__global__ void k_dump_hull(int obj, float *verts, int *faces, int *counts, float *normals, int *edges, float *local) {
    using namespace hs;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const HullRef h = obj == OBJ_WALL ? hull_ref_wall(0.f, 0.f, 1.f, 1.f) : hull_ref_body(obj, V3{0.f, 0.f, 0.f}, Q{1.f, 0.f, 0.f, 0.f});
    const int nv = hull_nv(h), nf = hull_nf(h), ne = hull_ne(h);
    counts[0] = nv; counts[1] = nf; counts[2] = ne; counts[3] = hull_ned(h);
    for (int i = 0; i < nv; ++i) {
        const V3 v = hull_v(h, i);
        verts[i * 3] = v.x; verts[i * 3 + 1] = v.y; verts[i * 3 + 2] = v.z;
        const V3 l = obj == OBJ_WALL ? V3{0.f, 0.f, 0.f} : hull_local_vertex(obj, i);
        local[i * 3] = l.x; local[i * 3 + 1] = l.y; local[i * 3 + 2] = l.z;
    }
    for (int f = 0; f < nf; ++f) {
        for (int k = 0; k < 4; ++k) faces[f * 4 + k] = k < hull_fcnt(h, f) ? hull_fidx(h, f, k) : -1;
        const V3 n = hull_fn(h, f);
        normals[f * 3] = n.x; normals[f * 3 + 1] = n.y; normals[f * 3 + 2] = n.z;
    }
    for (int e = 0; e < ne; ++e) { int v0, v1, d; hull_edge(h, e, &v0, &v1, &d); edges[e * 3] = v0; edges[e * 3 + 1] = v1; edges[e * 3 + 2] = d; }
}
int32_t hs_debug_dump_hull(int32_t obj, float *verts, int32_t *faces, int32_t *counts, float *normals, int32_t *edges, float *local) {
    if (!verts || !faces || !counts || !normals || !edges || !local) return fail(HS_ERR_INVALID_ARG, "null argument");
    if (obj != hs::OBJ_CUBE && obj != hs::OBJ_WALL && obj != hs::OBJ_HIDER && obj != hs::OBJ_SEEKER && obj != hs::OBJ_RAMP && obj != hs::OBJ_BOX)
        return fail(HS_ERR_INVALID_ARG, "no collision hull for this SimObject");
    char *d = nullptr;
    const size_t nb = (24 + 24 + 8 + 18 + 36 + 24) * 4;
    HS_HIP(hipMalloc((void **)&d, nb));
    HS_HIP(hipMemset(d, 0, nb));
    float *dv = (float *)d; int *df = (int *)(dv + 24), *dc = df + 24; float *dn = (float *)(dc + 8); int *de = (int *)(dn + 18); float *dl = (float *)(de + 36);
    hipLaunchKernelGGL(k_dump_hull, dim3(1), dim3(64), 0, nullptr, (int)obj, dv, df, dc, dn, de, dl);
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipMemcpy(verts, dv, 24 * 4, hipMemcpyDeviceToHost)); HS_HIP(hipMemcpy(faces, df, 24 * 4, hipMemcpyDeviceToHost));
    HS_HIP(hipMemcpy(counts, dc, 4 * 4, hipMemcpyDeviceToHost)); HS_HIP(hipMemcpy(normals, dn, 18 * 4, hipMemcpyDeviceToHost));
    HS_HIP(hipMemcpy(edges, de, 36 * 4, hipMemcpyDeviceToHost)); HS_HIP(hipMemcpy(local, dl, 24 * 4, hipMemcpyDeviceToHost));
    HS_HIP(hipFree(d));
    return HS_OK;
}

__global__ void k_object_params(int obj, float *out) {
    using namespace hs;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const V3 i = obj_inv_inertia(obj);
    out[0] = obj_inv_mass(obj); out[1] = obj_mu_s(obj); out[2] = obj_mu_d(obj); out[3] = i.x; out[4] = i.y; out[5] = i.z;
}
int32_t hs_debug_object_params(int32_t obj, float *out) {
    if (!out || obj < 0 || obj > hs::OBJ_BOX) return fail(HS_ERR_INVALID_ARG, "bad argument");
    float *d = nullptr;
    HS_HIP(hipMalloc((void **)&d, 6 * sizeof(float)));
    hipLaunchKernelGGL(k_object_params, dim3(1), dim3(64), 0, nullptr, (int)obj, d);
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipMemcpy(out, d, 6 * sizeof(float), hipMemcpyDeviceToHost));
    HS_HIP(hipFree(d));
    return HS_OK;
}

// hs_debug_core_eval: the scalar core's probe table (hs_core_probe.h) as the device compiler reads it, one case per lane.
// A template (like the kernels of hs_k_norm.h), so that the compiler emits it after the kernels there were before it and
// numbers their functions, and with them their branch labels, as before.
extern "C++" {
template <int kThreads>
__global__ void __launch_bounds__(kThreads) k_core_eval(int op, int n, const float *in, float *out) {
    using namespace hs;
    const int i = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
    if (i >= n) return;
    float x[kCoreWords], y[kCoreWords];
    for (int k = 0; k < kCoreWords; ++k) x[k] = in[(size_t)i * kCoreWords + k];
    core_eval(op, x, y);
    for (int k = 0; k < kCoreWords; ++k) out[(size_t)i * kCoreWords + k] = y[k];
}
}  // extern "C++"
int32_t hs_debug_core_eval(int32_t op, int32_t n, const float *in, float *out) {
    if (!in || !out || n <= 0 || n > (1 << 20) || op < 0 || op >= hs::CORE_NUM_OPS) return fail(HS_ERR_INVALID_ARG, "bad argument");
    const size_t nb = (size_t)n * hs::kCoreWords * sizeof(float);
    float *d = nullptr;
    HS_HIP(hipMalloc((void **)&d, 2 * nb));
    HS_HIP(hipMemcpy(d, in, nb, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_core_eval<256>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, (int)op, (int)n, (const float *)d, d + (size_t)n * hs::kCoreWords);
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipMemcpy(out, d + (size_t)n * hs::kCoreWords, nb, hipMemcpyDeviceToHost));
    HS_HIP(hipFree(d));
    return HS_OK;
}

// DLPack deleter for the non-owning tensor views handed to Python: the simulator owns the memory, the
// binding keeps the DLManagedTensor records alive, so there is nothing to free (and nothing here may call
// back into an interpreter that is shutting down).
void hs_dlpack_noop_deleter(void *) {}

int32_t hs_train_interface(const hs_iface_entry **entries) {
    if (entries) *entries = kTrainInterface;
    return (int32_t)(sizeof(kTrainInterface) / sizeof(kTrainInterface[0]));
}

int32_t hs_get_device_status(hs_sim *s, hs_device_status *out) {
    HS_ENTER(s && out, "null argument");
    HS_HIP(hipDeviceSynchronize());
    int st[4];
    HS_HIP(hipMemcpy(st, s->S.status, sizeof(st), hipMemcpyDeviceToHost));
    out->split_steps = s->split_steps;
    out->late_octets = (uint32_t)st[2];
    out->spilled_dd_pairs = st[0];
    out->spilled_static_pairs = st[1];
    out->dropped_dd_pairs = 0;             // nothing can overflow the spill lists (hs_k_physics.h: sized for every pair)
    out->dropped_static_pairs = 0;
    out->graphs_in_use = 0;                // (HIP-graph replay was removed)
    out->reserved = 0;
    return HS_OK;
}

int32_t hs_set_late_threshold(hs_sim *s, float factor) {
    if (!s) return fail(HS_ERR_INVALID_ARG, "null sim");
    if (!(factor >= 0.f)) return fail(HS_ERR_INVALID_ARG, "hs_set_late_threshold: the factor must be >= 0");
    HS_HIP(hipSetDevice(s->cfg.gpu_id));
    const float f = factor < kMaxLateFactor ? factor : kMaxLateFactor;
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipMemcpy(hs::sched_words(s->S) + hs::kSchedFactor, &f, 4, hipMemcpyHostToDevice));
    return HS_OK;
}

int32_t hs_set_profiling(hs_sim *s, int32_t enabled) {
    if (!s) return fail(HS_ERR_INVALID_ARG, "null sim");
    s->profiling = enabled != 0;
    return HS_OK;
}

int32_t hs_last_step_kernel_ms(hs_sim *s, float out_ms[3]) {
    if (!s || !out_ms) return fail(HS_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < 3; ++i) out_ms[i] = s->last_ms[i];
    return HS_OK;
}

}  // extern "C"

// ---- the gradient reduction (hs_k_reduce.h): its launch, the last kernel the file names ----
namespace {
int launch_reduce(hs_sim *, hipStream_t strm, const hs_grad_reduce_request *r) {
    hs::ReduceArgs a = {};
    for (int g = 0; g < r->shards; ++g) a.src[g] = r->src[g];
    a.count = r->count; a.dst = r->dst; a.total = r->total; a.n = (int)r->n; a.shards = r->shards;
    hipLaunchKernelGGL(hs::k_reduce<>, dim3(hs::adam_grid(a.n, hs::kAdamStepMaxGrid)), dim3(hs::kAdamThreads), 0, strm, a);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace

// ---- the SimHash encoder (hs_k_hash.h): its launches, after every kernel the file named before ----
namespace {
// One k_hash_fwd over the rows (the request has passed check_hash).
int launch_hash(hs_sim *, hipStream_t strm, const hs_hash_encode_request *r) {
    hs::HashArgs a = {};
    a.rows = r->rows; a.params = r->params; a.features = r->features; a.bin = r->bin;
    a.n = r->n; a.rowsType = elem_code(r->rows_dtype); a.featType = elem_code(r->features_dtype); a.eps = r->eps;
    hipLaunchKernelGGL(hs::k_hash_fwd<>, dim3(hs::rows_grid(a.n, hs::kHashRows, hs::kHashMaxGrid)), dim3(hs::kRowsThreads), 0, strm, a);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// k_hash_bwd_bins into the workspace's slices, their fixed-order sum into its last slice, and k_hash_bwd_table from there
// (the request has passed check_hash_bwd).
int launch_hash_bwd(hs_sim *s, hipStream_t strm, const hs_hash_encode_backward_request *r) {
    hs::HashBwdArgs a = {};
    a.bin = r->bin; a.gradFeatures = r->grad_features; a.params = r->params; a.workspace = s->hash_partials; a.gradParams = r->grad_params;
    a.n = r->n; a.gradType = elem_code(r->grad_dtype); a.eps = r->eps;
    const int nparts = hs::rows_grid(a.n, hs::kHashRows, hs::kHashMaxGridBwd);
    float *G = s->hash_partials + (size_t)hs::kHashMaxGridBwd * hs::kHashSlice;
    hipLaunchKernelGGL(hs::k_hash_bwd_bins<>, dim3(nparts), dim3(hs::kRowsThreads), 0, strm, a);
    launch_partials_sum<float, hs::kRowsSumCols, hs::kRowsSumSegs>(strm, s->hash_partials, nparts, hs::kHashSlice, G);
    hipLaunchKernelGGL(hs::k_hash_bwd_table<>, dim3(1), dim3(hs::kRowsThreads), 0, strm, a, (const float *)G);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
}  // namespace
