/*
 * hideseek.h — C ABI of the MI355X-native batch hide-and-seek simulator (libhideseek.so).
 *
 * This is the drop-in boundary for the reference's `Manager` class (src/mgr.hpp:14-99): one opaque
 * simulator handle per shard of worlds, `init` / `step`, and non-owning descriptors of the
 * exported columns that the reference hands to Python as `madrona::py::Tensor`
 * (src/mgr.cpp:824-842, 1062-1336).  No C++ or torch types cross this boundary: plain pointers,
 * sizes and status codes.  Errors are returned as status codes instead of the reference's
 * FATAL()/abort (src/mgr.cpp:466,573,762); `hs_last_error()` gives the message.
 *
 * All tensors live in device (HBM) memory of `gpu_id`, are row-major contiguous and stay valid
 * and at the same address until `hs_destroy` (src/mgr.hpp ownership convention; the scripts write
 * `action` and `reset` in place: scripts/benchmark.py:64-65,82-84).
 */
#ifndef HIDESEEK_H
#define HIDESEEK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hs_sim hs_sim;   /* replaces Manager::Impl (src/mgr.hpp:94-98) */

/* Status codes (the reference aborts instead). */
enum {
    HS_OK = 0,
    HS_ERR_INVALID_ARG = 1,
    HS_ERR_NO_DEVICE = 2,      /* no HIP device / HIP runtime failure */
    HS_ERR_UNSUPPORTED = 3,    /* e.g. exec_mode CPU: this library has no CPU execution path */
    HS_ERR_HIP = 4
};

/* madrona::ExecMode as used by Manager::Config::execMode (src/mgr.hpp:17). */
enum { HS_EXEC_CPU = 0, HS_EXEC_GPU = 1 /* "CUDA" in the reference's Python enum */ };

/* SimFlags (src/sim_flags.hpp:7-13). Bits 16+ are build-side extensions. */
enum {
    HS_FLAG_DEFAULT = 0,
    HS_FLAG_USE_FIXED_WORLD = 1 << 0,
    HS_FLAG_IGNORE_EPISODE_LENGTH = 1 << 1,
    HS_FLAG_RANDOM_FLIP_TEAMS = 1 << 2,
    HS_FLAG_ZERO_AGENT_VELOCITY = 1 << 3,
    /* extension: skip the observation task-graph nodes (sim.cpp:1232-1293) — the physics-only
       roofline configuration of BASELINE.json configs[2]; not a reference flag. */
    HS_FLAG_EXT_SKIP_OBSERVATIONS = 1 << 16,
    /* extension: render the agent views (depth + RGB, hs_render below) as part of every init / step when
       enable_batch_renderer is set.  Without it the renderer outputs stay allocated and unwritten, which is what the
       reference scripts' arguments get (scripts/benchmark.py:32,47 only takes the tensor). */
    HS_FLAG_EXT_RENDER = 1 << 17
};

/* Manager::Config (src/mgr.hpp:16-32) + the shard placement of SURVEY §8e. */
typedef struct hs_config {
    int32_t exec_mode;            /* HS_EXEC_GPU */
    int32_t gpu_id;               /* Manager::Config::gpuID */
    int32_t num_worlds;           /* worlds simulated by THIS handle */
    uint32_t sim_flags;
    uint32_t rand_seed;
    int32_t min_hiders, max_hiders, min_seekers, max_seekers;
    int32_t num_pbt_policies;
    int32_t enable_batch_renderer;   /* rgb/depth tensors; rendered by hs_render / under HS_FLAG_EXT_RENDER */
    int32_t batch_render_width, batch_render_height;
    int32_t world_offset;         /* global index of local world 0 (RNG keys use global ids) */
} hs_config;

/* ExportID (src/sim.hpp:45-68), same numbering, plus the two renderer outputs
 * (src/mgr.cpp:1241-1263) and debug dumps of internal state used by the parity tests. */
enum {
    HS_EXPORT_RESET = 0,
    HS_EXPORT_PREP_COUNTER = 1,
    HS_EXPORT_ACTION = 2,
    HS_EXPORT_SELF_OBS = 3,
    HS_EXPORT_SELF_TYPE = 4,
    HS_EXPORT_SELF_MASK = 5,
    HS_EXPORT_AGENT_OBS = 6,
    HS_EXPORT_BOX_OBS = 7,
    HS_EXPORT_RAMP_OBS = 8,
    HS_EXPORT_AGENT_VIS_MASKS = 9,
    HS_EXPORT_BOX_VIS_MASKS = 10,
    HS_EXPORT_RAMP_VIS_MASKS = 11,
    HS_EXPORT_LIDAR = 12,
    HS_EXPORT_SEED = 13,
    HS_EXPORT_REWARD = 14,
    HS_EXPORT_DONE = 15,
    HS_EXPORT_GLOBAL_DEBUG_POSITIONS = 16,
    HS_EXPORT_AGENT_POLICY = 17,
    HS_EXPORT_EPISODE_RESULT = 18,
    HS_EXPORT_CHECKPOINT_CONTROL = 19,
    HS_EXPORT_CHECKPOINT = 20,
    HS_EXPORT_DEPTH = 21,
    HS_EXPORT_RGB = 22,
    HS_NUM_EXPORTS = 23
};

/* Element types.  HS_DTYPE_BF16 / HS_DTYPE_F16 are output types of hs_pack_policy_inputs, logits types of
 * hs_sample_actions, value types of hs_compute_gae and the types of hs_ppo_loss only: no export has them. */
enum { HS_DTYPE_I32 = 0, HS_DTYPE_F32 = 1, HS_DTYPE_U8 = 2, HS_DTYPE_BF16 = 3, HS_DTYPE_F16 = 4 };

/* madrona::py::Tensor (src/mgr.cpp:824-842): pointer, element type, dimensions, device. */
typedef struct hs_tensor_desc {
    void *ptr;
    int32_t dtype;
    int32_t ndim;
    int64_t dims[4];
    int32_t gpu_id;
} hs_tensor_desc;

/* Checkpoint (src/sim.hpp:283-313): the per-world snapshot behind `ckpt_tensor()` ([N, 1392] u8) and the
 * replay log of scripts/jax_infer.py:125.  Field order follows the reference struct; Quat is w,x,y,z,
 * Velocity is linear then angular.  The engine's JointConstraint::Fixed is not in the reference tree:
 * {attachRot1, attachRot2, separation} is assumed, which reproduces the 1392-byte record. */
typedef struct hs_ckpt_object {          /* Checkpoint::DynObjectState (sim.hpp:294-297) */
    float pos[3], rot[4], lin[3], ang[3];
    uint32_t team;                        /* OwnerTeam: 0 None, 1 Seeker, 2 Hider, 3 Unownable (sim.hpp:127-132) */
    uint8_t is_locked, _pad[3];
} hs_ckpt_object;
typedef struct hs_ckpt_agent {           /* Checkpoint::AgentState (sim.hpp:299-304) */
    float pos[3], rot[4], lin[3], ang[3];
    int32_t grab_idx;                     /* box index, or numBoxes + ramp index, or -1 */
    float grab_r1[3], grab_r2[3];
    float attach_rot1[4], attach_rot2[4], separation;
} hs_ckpt_agent;
typedef struct hs_checkpoint {
    uint32_t episode_key[2];              /* curEpisodeRNDCounter = {episode index, world id} */
    int32_t running_scores[2];            /* EpisodeStats (sim.hpp:109-111) */
    int32_t episode_step;
    hs_ckpt_agent agents[6];              /* hiders, then seekers */
    hs_ckpt_object boxes[9];
    hs_ckpt_object ramps[2];
    int32_t num_hiders, num_seekers, num_boxes, num_ramps;
} hs_checkpoint;

/* Manager::Manager (src/mgr.cpp:844-846 -> Impl::make :674-822). */
int32_t hs_create(const hs_config *cfg, hs_sim **out);
/* Manager::~Manager (src/mgr.cpp:848-859). */
void hs_destroy(hs_sim *sim);
/* Manager::init (src/mgr.cpp:861-881): runs the Init task graph (sim.cpp:1295-1305); blocking. */
int32_t hs_init(hs_sim *sim);
/* Manager::step (src/mgr.cpp:883-903): runs the Step task graph once (sim.cpp:1307-1313); blocking. */
int32_t hs_step(hs_sim *sim);
/* The two halves of hs_step, for a front-end that owns several handles (one per GPU of the node): every
 * handle has its own HIP stream; hs_step_begin orders that stream after the work already queued on the device's
 * legacy default stream (where torch writes `action`), enqueues the step and returns; hs_step_end waits for it and
 * reports device-side failures (hs_get_device_status).  hs_step == hs_step_begin + hs_step_end.  The reference is
 * single-GPU (src/mgr.hpp:18); these replace the executor's run() for the sharded case. */
int32_t hs_step_begin(hs_sim *sim);
int32_t hs_step_end(hs_sim *sim);
/* Manager::gpuJAXStep / CUDAImpl::gpuStreamStep (src/mgr.cpp:379-398, 1006-1022): enqueue one step on a
 * caller-supplied hipStream_t (passed as void*) without synchronising. */
int32_t hs_step_async(hs_sim *sim, void *hip_stream);

/* Render every agent's view of the current state into the depth / rgb exports (Manager::step's
 * renderMgr->batchRender(), src/mgr.cpp:894-901, with the camera of src/sim.cpp:1400-1403: 100 degrees vertical field
 * of view, z-near 0.001, 0.5 above the agent's origin, looking along the agent's forward axis).  depth [N*A,H,W,1] f32
 * = view-space depth of the closest hit (0: nothing hit / inactive agent); rgb [N*A,H,W,4] u8 = base colour of the hit
 * object (src/mgr.cpp:621-647, textures not reproduced) x (0.3 + 0.7 Lambert term of the light of :657-659), alpha 255.
 * Blocking.  Madrona's renderer is absent from the reference snapshot: the image is this build's own. */
int32_t hs_render(hs_sim *sim);

/* Spectator cameras (the function of the reference's src/viewer.cpp without a window): render any world of this handle
 * from any pose.  Axes as the agent camera's: local +y forward, +x right, +z up; rot = w,x,y,z, used as given (no
 * normalisation).  A pixel is hs_render's pixel with tan_half_fov_y in place of tan(50 degrees): a camera at an agent's
 * pose + (0, 0, 0.5) with tan_half_fov_y = tan(50 degrees) reproduces that agent's view bit for bit. */
typedef struct hs_camera {
    int32_t world;                /* local world index of this handle */
    float pos[3];
    float rot[4];
    float tan_half_fov_y;
} hs_camera;
enum { HS_SPECTATE_NO_CULL = 1 };  /* test every pixel against everything (the culls are conservative: same output) */
/* Render `n` cameras (`cams`: host memory) at width x height into caller-owned device buffers of this handle's GPU:
 * depth [n,H,W] f32 (0: nothing hit), rgba [n,H,W,4] u8 (alpha 255, black sky), hit [n,H,W] i32 (0-16 movable body
 * slot, 100+k wall k, 200+p plane p, -1 nothing or nearer than z-near).  Any output may be null, not all three; each
 * must be 4-byte aligned.  Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written):
 * world in [0, num_worlds), 1 <= width, height <= 4096, n >= 1, a finite pose, |rot|^2 in [0.99, 1.01], tan_half_fov_y
 * finite and > 0.  Refused before hs_init and inside an open step; ordered after the device's legacy default stream;
 * blocking.  Writes no simulator state; works without enable_batch_renderer and under HS_FLAG_EXT_SKIP_OBSERVATIONS. */
int32_t hs_render_cameras(hs_sim *sim, const hs_camera *cams, int32_t n, int32_t width, int32_t height, uint32_t flags,
                          float *depth, uint8_t *rgba, int32_t *hit);
/* The 21 Manager::*Tensor() getters + policyAssignmentsTensor / episodeResultTensor
 * (src/mgr.cpp:1062-1336). */
int32_t hs_get_tensor(hs_sim *sim, int32_t export_id, hs_tensor_desc *out);
/* Manager::triggerReset (src/mgr.cpp:1265-1281). */
int32_t hs_trigger_reset(hs_sim *sim, int32_t world_idx, int32_t level_idx);
/* Manager::setAction (src/mgr.cpp:1283-1305). */
int32_t hs_set_action(hs_sim *sim, int32_t agent_idx, int32_t x, int32_t y, int32_t r, int32_t g, int32_t l);
/* Manager::saveCheckpoint (src/mgr.cpp:905-929): set world's CheckpointControl trigger, run the
 * SaveCheckpoints graph (sim.cpp:1315-1322: every triggered world writes its hs_checkpoint and clears the
 * trigger); blocking. */
int32_t hs_save_checkpoint(hs_sim *sim, int32_t world_idx);
/* Manager::loadCheckpoint (src/mgr.cpp:931-963): set the trigger, run the LoadCheckpoints graph. */
int32_t hs_load_checkpoint(hs_sim *sim, int32_t world_idx);
/* Manager::loadCheckpoints (src/mgr.cpp:965-985): run the LoadCheckpoints graph (sim.cpp:1324-1333) for
 * the triggers currently in the ckpt_ctrl tensor: triggered worlds regenerate their level from the saved
 * episode key and restore body / joint / episode state (sim.cpp:956-1044, trigger left at 1 as :963 does);
 * then observations are recomputed for all worlds. */
int32_t hs_load_checkpoints(hs_sim *sim);
/* CUDAImpl::saveCheckpoints (src/mgr.cpp:316-319): run the SaveCheckpoints graph for the current triggers. */
int32_t hs_save_checkpoints(hs_sim *sim);

/* Policy inputs: what the reference's policy makes of the observation exports before its network sees them
 * (scripts/jax_policy.py:84-98 extract_self_obs, :262-280 the actor's tables, :372-390 the critic's), as one row of
 * HS_PACK_ROW features per agent row (world * A + slot), written in the learner's element type into the learner's memory:
 *   column 0        (float)prep_counter / 96.0f              (jax_policy.py:86)
 *   columns 1-13    self_data;  14: (float)self_type;  15-44: lidar       (the "self" row, jax_policy.py:88-98)
 *   columns 45-114  agent_data [5][14];  115-267: box_data [9][17];  268-295: ramp_data [2][14]
 * critic: the data as exported (jax_policy.py:372-390).  actor: columns 45-295 are data * visibility mask of the entity,
 * an IEEE f32 multiplication (jax_policy.py:262-280: agent_data * vis_agents_mask, ...).  HS_DTYPE_BF16 / HS_DTYPE_F16
 * round the f32 value to nearest even (jnp.astype, jax_policy.py:84; f16 subnormals kept, beyond 65504: infinity).
 * moments [HS_PACK_MOMENTS] f64, for an observation normaliser: with m = self_mask of the row (1.0 or 0.0,
 * src/level_gen.cpp:21, 332) and x the f32 critic value of column c: [c] = sum m x, [HS_PACK_ROW + c] = sum m x x,
 * [2 HS_PACK_ROW] = sum m, over all rows.  Summed without atomics in an order that depends on the row count alone: the
 * same state gives the same bits on every call.  The partial sums go through a workspace of the handle, so two calls
 * with moments on one handle must not overlap.
 * Outputs are caller-owned device memory of the handle's GPU: contiguous [rows][HS_PACK_ROW], 16-byte aligned.  Any may
 * be null, not all three.  Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written):
 * null request, every output null, unknown dtype, misaligned pointer.  HS_ERR_INVALID_ARG before hs_init and inside an
 * open step; HS_ERR_UNSUPPORTED under HS_FLAG_EXT_SKIP_OBSERVATIONS (there are no observations).  Writes no simulator
 * state.  hs_pack_policy_inputs is ordered after the device's legacy default stream and blocking;
 * hs_pack_policy_inputs_async enqueues on the caller's hipStream_t without synchronising, as hs_jax_step does (the
 * caller orders it after the step that wrote the observations). */
enum { HS_PACK_ROW = 296, HS_PACK_MOMENTS = 593 };
typedef struct hs_pack_request {
    void *actor;                  /* [rows][HS_PACK_ROW] of actor_dtype, or null */
    int32_t actor_dtype;          /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    void *critic;
    int32_t critic_dtype;
    double *moments;              /* [HS_PACK_MOMENTS], or null */
} hs_pack_request;
int32_t hs_pack_policy_inputs(hs_sim *sim, const hs_pack_request *req);
int32_t hs_pack_policy_inputs_async(hs_sim *sim, void *hip_stream, const hs_pack_request *req);

/* Observation normaliser: the exponential moving average that the reference's policy wraps around its network
 * (scripts/jax_policy.py:372-390, ObservationsEMANormalizer.create(decay = 0.99999, ...)), kept on the device between a
 * rollout and the next pack.  It normalises every column of the row but HS_NORM_SKIP_PREP_COUNTER and
 * HS_NORM_SKIP_SELF_TYPE (jax_policy.py:382-389 leaves prep_counter, self_type and the masks alone; the masks are not
 * columns of the row).  madrona_learn is not available, so the update rule below is this project's contract and is not
 * pinned to the reference's.
 * state [HS_NORM_STATE] f64, caller-owned device memory: m1[c] = [c] the running first moment of column c,
 * m2[c] = [HS_PACK_ROW + c] the running second raw moment, N = [2 HS_PACK_ROW] the bias-correction weight.  All zeros is
 * a fresh normaliser.
 * table [HS_NORM_TABLE] f32, caller-owned device memory, 16-byte aligned: mu[c] = [c], inv[c] = [HS_PACK_ROW + c]; what
 * hs_pack_policy_inputs_normalized reads.
 * hs_obs_norm_update, one kernel (csrc/hs_k_norm.h).  The num_moments vectors of `moments` (each as
 * hs_pack_policy_inputs writes it: several shards, or the T steps of a rollout) form one batch.  IEEE f64, unfused, in
 * exactly this order:
 *   s1[c], s2[c], n = the sums of the vectors' [c], [HS_PACK_ROW + c], [2 HS_PACK_ROW], added in index order starting
 *                     from the first vector
 *   if n > 0, with a = 1.0 - decay:    m1[c] = decay * m1[c] + a * (s1[c] / n)
 *                                      m2[c] = decay * m2[c] + a * (s2[c] / n)
 *                                      N     = decay * N + a                   (two products and one addition each)
 *   otherwise the state is unchanged.
 *   The table is always rewritten from the resulting state.  A normalised column with N > 0:
 *       mu = m1[c] / N;   v = m2[c] / N - mu * mu;   v = v < 0 ? 0 : v        (a select)
 *       table[c] = (float)mu;   table[HS_PACK_ROW + c] = (float)(1.0 / sqrt(v + eps))
 *   A skipped column, or N == 0:  table[c] = +0.0f;   table[HS_PACK_ROW + c] = 1.0f.
 * No atomics: the result depends on the inputs alone.  Everything is validated before anything is launched
 * (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a null request; null moments, state or table;
 * num_moments outside [1, HS_NORM_MAX_MOMENTS]; decay outside [0, 1) or NaN; eps not finite or <= 0; moments or state
 * not 8-byte aligned, a table not 16-byte aligned; state or table overlapping moments or each other; a call before
 * hs_init or inside an open step.  It reads no export and writes no simulator state; the handle supplies the device.
 * hs_obs_norm_update is ordered after the device's legacy default stream and blocking; hs_obs_norm_update_async enqueues
 * on the caller's hipStream_t without synchronising. */
enum { HS_NORM_STATE = 593, HS_NORM_TABLE = 592, HS_NORM_MAX_MOMENTS = 4096 };
enum { HS_NORM_SKIP_PREP_COUNTER = 0, HS_NORM_SKIP_SELF_TYPE = 14 };      /* the columns that are not normalised */
typedef struct hs_obs_norm_request {
    const double *moments;        /* [num_moments][HS_PACK_MOMENTS] f64, contiguous */
    int32_t num_moments;          /* 1 .. HS_NORM_MAX_MOMENTS */
    double decay;                 /* in [0, 1) */
    double eps;                   /* finite, > 0 */
    double *state;                /* [HS_NORM_STATE] f64, read and written */
    float *table;                 /* [HS_NORM_TABLE] f32, written */
} hs_obs_norm_request;            /* 48 bytes */
int32_t hs_obs_norm_update(hs_sim *sim, const hs_obs_norm_request *req);
int32_t hs_obs_norm_update_async(hs_sim *sim, void *hip_stream, const hs_obs_norm_request *req);

/* hs_pack_policy_inputs with the normaliser's table (one kernel, k_pack_norm).  Everything hs_pack_policy_inputs
 * specifies still holds; in addition every element of the critic row is y = (x - mu[c]) * inv[c], one IEEE f32
 * subtraction then one f32 multiplication, unfused, on the f32 value x of the un-normalised critic row; the actor row is
 * y * mask in columns 45-295 (normalise, then mask, as the reference's obs_preprocess runs before ActorNet); the cast to
 * the output type comes last.  The moments stay those of the raw x, so one launch normalises with the current table
 * and collects the statistics of the next update.  With the table of a fresh state, (x - 0) * 1, the outputs have the
 * bits of hs_pack_policy_inputs, -0 included.  Validation, ordering and streams as hs_pack_policy_inputs; a null or
 * not 16-byte aligned table is refused with HS_ERR_INVALID_ARG before anything is launched.  The table is read by the
 * kernel: an hs_obs_norm_update that rewrites it must be ordered before or after the pack. */
int32_t hs_pack_policy_inputs_normalized(hs_sim *sim, const hs_pack_request *req, const float *table);
int32_t hs_pack_policy_inputs_normalized_async(hs_sim *sim, void *hip_stream, const hs_pack_request *req, const float *table);

/* Action sampling: the leg after the network.  The actor's logits of every agent row (world * A + slot) become the
 * [rows][HS_SAMPLE_HEADS] i32 action the next hs_step reads, with the log-probability and the entropy a PPO learner
 * stores, in one kernel (csrc/hs_k_sample.h) — a multi-discrete actor head as the reference's learner has it
 * (scripts/jax_train.py:146-148, actions_num_buckets = [5, 5, 5, 2, 2]).
 * A row has L = sum of buckets[h] logits, head after head, at logits + row * logits_stride (in elements) of
 * logits_dtype (HS_DTYPE_F32 | _BF16 | _F16; narrow types are widened to f32 exactly, all arithmetic is IEEE f32
 * without contraction, expf / logf are the accurate library functions).  Head h with K = buckets[h] logits l_0 .. l_{K-1}:
 *   m = max l_i;   e_i = expf(l_i - m);   c_i = ((e_0 + e_1) + ...) + e_i, added in index order;   S = c_{K-1}
 *   log_prob_h = (l_a - m) - logf(S)
 *   entropy_h  = logf(S) - (sum_i e_i * (l_i - m)) / S     summed in index order; a term with e_i == 0 is exactly 0
 * A logit of -inf masks its bucket (e_i = 0) and produces no NaN; a head needs one finite logit, +inf and NaN are not
 * supported.  The action a of the head:
 *   HS_SAMPLE_DRAW      the smallest index with u * S < c_a (an f32 product); if there is none, the last index with
 *                       e_i > 0.  A bucket with e_i == 0 is never drawn.
 *   HS_SAMPLE_GREEDY    the first index of the maximum logit.
 *   HS_SAMPLE_EVALUATE  the value stored in the action buffer, clamped into [0, K) for the lookup; the action buffer
 *                       is only read.
 * The uniform u of (row, head h): with g = (world_offset + world) * A + slot, the global agent row,
 *   k = threefry2x32(key = {seed[0], seed[1]}, c0 = g, c1 = counter)         (Threefry-2x32-20)
 *   {x0, x1} = threefry2x32(key = k, c0 = h, c1 = 0);   u = (float)((x0 ^ x1) >> 8) * 2^-24      in [0, 1)
 * so a draw depends on seed, counter and the global row alone: handles that split the worlds between them
 * (world_offset) draw what one handle over all of them draws.  Use a fresh counter (or seed) for every call of a rollout.
 * Row outputs: log_prob = (((lp_0 + lp_1) + lp_2) + lp_3) + lp_4 and entropy likewise, in this order; head_log_prob
 * holds the five lp_h.  HS_SAMPLE_ZERO_INACTIVE: a row whose self_mask export is 0 gets action 0 in every head and 0 in
 * log_prob, entropy and head_log_prob (in HS_SAMPLE_EVALUATE its action is left as it is).
 * action, log_prob, entropy, head_log_prob: contiguous device memory of the handle's GPU, 4-byte aligned; logits
 * aligned to their element size.  Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing
 * written): null request or logits, unknown dtype, mode or flag bit, a bucket count outside [1, HS_SAMPLE_MAX_BUCKETS],
 * more than HS_SAMPLE_MAX_LOGITS logits per row, logits_stride below the sum of the buckets, a misaligned pointer,
 * HS_SAMPLE_EVALUATE with every output null, a call before hs_init or inside an open step.  HS_SAMPLE_ZERO_INACTIVE
 * under HS_FLAG_EXT_SKIP_OBSERVATIONS: HS_ERR_UNSUPPORTED (no self_mask); without that flag the call works there.
 * Writes no simulator state but the action export, and that only with a null `action` outside HS_SAMPLE_EVALUATE.
 * hs_sample_actions is ordered after the device's legacy default stream and blocking, so a following hs_step sees the
 * actions; hs_sample_actions_async enqueues on the caller's hipStream_t without synchronising. */
enum { HS_SAMPLE_HEADS = 5, HS_SAMPLE_MAX_BUCKETS = 16, HS_SAMPLE_MAX_LOGITS = 64 };
enum { HS_SAMPLE_DRAW = 0, HS_SAMPLE_GREEDY = 1, HS_SAMPLE_EVALUATE = 2 };
enum { HS_SAMPLE_ZERO_INACTIVE = 1 };
typedef struct hs_sample_request {
    const void *logits;           /* [rows][logits_stride] of logits_dtype; the first sum-of-buckets columns are read */
    int32_t logits_dtype;         /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t logits_stride;        /* elements, >= sum of buckets */
    int32_t buckets[HS_SAMPLE_HEADS];     /* each in [1, HS_SAMPLE_MAX_BUCKETS] */
    int32_t mode;
    uint32_t flags;
    uint32_t seed[2];
    uint32_t counter;
    int32_t *action;              /* [rows][5]; null = the simulator's own action export, written in place */
    float *log_prob, *entropy;    /* [rows], either may be null */
    float *head_log_prob;         /* [rows][5] or null */
} hs_sample_request;
int32_t hs_sample_actions(hs_sim *sim, const hs_sample_request *req);
int32_t hs_sample_actions_async(hs_sim *sim, void *hip_stream, const hs_sample_request *req);

/* Advantages and value targets: the leg after the last step of a rollout.  Generalised advantage estimation as the
 * reference trains with it (scripts/jax_train.py:45,152-153: gamma 0.998, gae_lambda 0.95, 40 steps per update) over the
 * rewards, dones and critic values of T steps, in one kernel (csrc/hs_k_gae.h).  Every array is [T][rows], rows =
 * num_worlds * A of the handle (row = world * A + slot), contiguous; every pointer is device memory of the handle's GPU.
 * The arithmetic is the contract.  Narrow values (HS_DTYPE_BF16 / _F16) are widened to f32 exactly; everything is IEEE
 * f32, unfused, in exactly this order.  Per row, with gl = gamma * lambda (an f32 product) and carry = 0, for t = T-1
 * down to 0:
 *   v      = value[t];   vn = (t == T-1) ? bootstrap : value[t+1]
 *   active = mask == null || mask[t] != 0;      ended = done[t] != 0
 *   if !active:  adv = +0.0, ret = +0.0, carry = +0.0        (selects: reward / value / vn of this step are not used, a
 *                                                             NaN there reaches no output)
 *   else:        delta = ended ? (reward[t] - v) : ((reward[t] + gamma * vn) - v)
 *                adv   = ended ? delta : (delta + gl * carry)
 *                ret   = adv + v;   carry = adv
 *   advantage[t] = adv;  returns[t] = ret
 * On an ended step vn and carry are selected away, not multiplied by zero: a NaN in the next episode's first value does
 * not leak backwards.  The done of the 240-step episode limit is terminal, as the reference treats it.
 * moments [HS_GAE_MOMENTS] f64, over the active (t, row) pairs: [0] = sum adv, [1] = sum adv^2, [2] = sum ret,
 * [3] = sum ret^2, [4] = their count; each term is the f64 of the f32 value, the square is taken in f64.  Summed without
 * atomics in an order that depends on (rows, T) alone: the same inputs give the same bits on every call.  The partial
 * sums go through a workspace of the handle, so two calls with moments on one handle must not overlap.
 * advantage, returns and moments may each be null, not all three; only what is requested is written.  Everything is
 * validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a null request;
 * a null reward, done, value or bootstrap; every output null; an unknown value_dtype; steps outside
 * [1, HS_GAE_MAX_STEPS]; gamma or lambda not finite or outside [0, 1]; a pointer not aligned to its element size
 * (moments: 8 bytes); an output range that overlaps an input range or another output; a call before hs_init or inside an
 * open step.  It reads no export itself, so it works under HS_FLAG_EXT_SKIP_OBSERVATIONS, and writes no simulator state.
 * hs_compute_gae is ordered after the device's legacy default stream and blocking; hs_compute_gae_async enqueues on the
 * caller's hipStream_t without synchronising. */
enum { HS_GAE_MAX_STEPS = 4096, HS_GAE_MOMENTS = 5 };
typedef struct hs_gae_request {
    const float   *reward;        /* [T][rows] f32: the reward export of step t */
    const int32_t *done;          /* [T][rows] i32: the done export of step t; nonzero = the episode ended with step t */
    const void    *value;         /* [T][rows] of value_dtype: V(observation the action of step t was chosen from) */
    const void    *bootstrap;     /* [rows] of value_dtype: V(observation after step T-1) */
    const float   *mask;          /* [T][rows] f32 (the self_mask export at step t: 1.0 / 0.0), or null = all active */
    int32_t value_dtype;          /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t steps;                /* T, 1 .. HS_GAE_MAX_STEPS */
    float gamma, lambda;          /* each finite, in [0, 1] */
    float  *advantage;            /* [T][rows] f32 or null */
    float  *returns;              /* [T][rows] f32 or null */
    double *moments;              /* [HS_GAE_MOMENTS] f64 or null */
} hs_gae_request;                 /* 80 bytes */
int32_t hs_compute_gae(hs_sim *sim, const hs_gae_request *req);
int32_t hs_compute_gae_async(hs_sim *sim, void *hip_stream, const hs_gae_request *req);

/* The PPO loss and its gradients: the leg after the network's forward pass of a minibatch.  Over n samples (a sample is
 * one (step, agent row) pair; n is free, it is not tied to the handle's rows, which supplies the device and a workspace)
 * one kernel (csrc/hs_k_ppo.h) reads the new logits and value, the stored action, old log-probability, advantage and
 * return once and writes d loss / d logits, d loss / d value and the sums behind the loss statistics once: the clipped
 * surrogate, the (optionally clipped) value loss and the entropy bonus as the reference's learner has them
 * (scripts/jax_train.py:41-45), with their closed-form gradients, so that the learner calls backward on the network's
 * outputs with these gradients and no autograd graph of the loss exists.
 * The arithmetic is the contract.  Narrow logits and values are widened to f32 exactly; everything is IEEE f32, unfused,
 * in exactly this order; expf / logf are the accurate library functions.  sum5(x) = (((x_0 + x_1) + x_2) + x_3) + x_4.
 * Head h of a sample, with K = buckets[h] logits l_i and the action a_h clamped into [0, K): m, e_i = expf(l_i - m), S,
 * log_prob_h and entropy_h exactly as hs_sample_actions defines them (HS_SAMPLE_EVALUATE), and logS = logf(S).
 *   lp = sum5(log_prob_h);  ent = sum5(entropy_h)       the bits hs_sample_actions returns under the same logits
 *   A  = advantage, or with adv_moments M (the moments of hs_compute_gae): (advantage - mean) / (std + 1e-8f), where in
 *        f64 mu = M[0] / M[4], mean = (float)mu, std = (float)sqrt(max(M[1] / M[4] - mu * mu, 0)); both 0 when M[4] == 0
 *   dlp = lp - old_log_prob;  ratio = expf(dlp);  s1 = ratio * A;  s2 = min(max(ratio, 1.f - c), 1.f + c) * A
 *   pg = s1 <= s2 ? -s1 : -s2;     g_lp = s1 <= s2 ? -s1 : +0;     kl = (ratio - 1.f) - dlp          (c = clip_coef)
 *   with value (v the new value, R = returns):  dv = v - R
 *     old_value == null:  vl = 0.5f * (dv * dv);  g_v = dv
 *     else (vo = old_value):  dvo = v - vo;  dvc = |dvo| <= c ? dv : (vo + (dvo < 0 ? -c : c)) - R     (inside the clip
 *                         range the clipped value is v itself, not vo + (v - vo) with its rounding: u2 == u1 there)
 *                         u1 = dv * dv;  u2 = dvc * dvc;  vl = 0.5f * (u1 >= u2 ? u1 : u2);   g_v = u1 >= u2 ? dv : +0
 *   active = mask == null || mask != 0;   cnt = the number of active samples, counted on the device before the
 *   gradients are made;   w = grad_scale / (float)cnt
 *   bucket i of head h:  d = l_i - m;  p = e_i / S;  t = p * ((d - logS) + entropy_h)
 *                        x = g_lp * ((i == a_h ? 1.f : 0.f) - p) + entropy_coef * t;   y = w * x
 *                        grad_logits = (active && e_i > 0 && y != 0) ? y : +0
 *   grad_value:          y = w * (value_loss_coef * g_v);   grad_value = (active && y != 0) ? y : +0
 * These are selects: an inactive sample gets +0 everywhere whatever its inputs hold (a NaN there reaches no output), a
 * bucket without e_i > 0, such as one masked with -inf, gets exactly +0 (autograd through log_softmax gives NaN there), and
 * a zero of either sign is stored as +0.  As for hs_sample_actions a head needs one finite logit and +inf and NaN logits
 * are not supported; a head whose logits are all -inf has e_i = NaN and so gets +0 in every bucket, but the sample's
 * log-probability, and with it the gradients of its other heads and its terms of the statistics, are NaN.  grad_logits is rounded to grad_dtype to nearest even; only columns 0 .. L-1
 * of a row of grad_stride elements are written.  grad_value has value_dtype.  With cnt == 0 every gradient is +0.
 * stats [HS_PPO_STATS] f64, sums over the active samples of the f64 of the f32 per-sample values: [0] = sum pg,
 * [1] = sum vl (0 without value), [2] = sum ent, [3] = sum kl, [4] = the count of s2 < s1 (policy-clipped), [5] = the
 * count of u2 > u1 (value-clipped), [6] = cnt.  Summed without atomics in an order that depends on n alone: the same
 * inputs give the same bits on every call.  The gradients are those of
 *   loss = grad_scale * (stats[0] - entropy_coef * stats[2] + value_loss_coef * stats[1]) / cnt.
 * The count and the partial sums go through a workspace of the handle: two calls on one handle must not overlap.
 * grad_logits, grad_value and stats may each be null, not all three; only what is requested is written.  Everything is
 * validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a null request,
 * logits, action, old_log_prob or advantage; every output null; grad_value without value; value without returns; an
 * unknown dtype; a bucket count outside [1, HS_SAMPLE_MAX_BUCKETS] or more than HS_SAMPLE_MAX_LOGITS logits; a stride
 * below the sum of the buckets; n < 1 or n * stride >= 2^31; a coefficient that is not finite or clip_coef <= 0; a
 * pointer not aligned to its element size (adv_moments, stats: 8 bytes); an output range that overlaps an input range or
 * another output; a call before hs_init or inside an open step.  It reads no export and writes no simulator state, so it
 * works under HS_FLAG_EXT_SKIP_OBSERVATIONS.  hs_ppo_loss is ordered after the device's legacy default stream and
 * blocking; hs_ppo_loss_async enqueues on the caller's hipStream_t without synchronising. */
enum { HS_PPO_STATS = 7 };
typedef struct hs_ppo_request {
    const void    *logits;        /* [n][logits_stride] of logits_dtype: the new policy's logits */
    const int32_t *action;        /* [n][HS_SAMPLE_HEADS] i32: the stored actions */
    const float   *old_log_prob;  /* [n] f32: log_prob of hs_sample_actions when the action was drawn */
    const float   *advantage;     /* [n] f32 */
    const double  *adv_moments;   /* [HS_GAE_MOMENTS] f64 on the device (hs_compute_gae's moments), or null = as given */
    const float   *mask;          /* [n] f32 (self_mask: 1.0 / 0.0), or null = all active */
    const void    *value;         /* [n] of value_dtype: the new critic's value, or null = no value term */
    const float   *returns;       /* [n] f32; required iff value is given */
    const float   *old_value;     /* [n] f32, or null = the value loss is not clipped */
    int32_t n;                    /* samples, n >= 1 and n * stride < 2^31 */
    int32_t logits_dtype;         /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t logits_stride;        /* elements, >= sum of buckets */
    int32_t grad_dtype;           /* of grad_logits */
    int32_t grad_stride;          /* elements, >= sum of buckets */
    int32_t value_dtype;          /* of value and grad_value */
    int32_t buckets[HS_SAMPLE_HEADS];     /* as hs_sample_request */
    float clip_coef;              /* c > 0 */
    float value_loss_coef, entropy_coef, grad_scale;      /* finite */
    void   *grad_logits;          /* [n][grad_stride] of grad_dtype, or null */
    void   *grad_value;           /* [n] of value_dtype, or null */
    double *stats;                /* [HS_PPO_STATS] f64, or null */
} hs_ppo_request;                 /* 160 bytes */
int32_t hs_ppo_loss(hs_sim *sim, const hs_ppo_request *req);
int32_t hs_ppo_loss_async(hs_sim *sim, void *hip_stream, const hs_ppo_request *req);

/* The two-hot symlog critic head: the value leg of a learner whose critic emits a categorical distribution over B bins
 * in symlog space, as the reference trains it (scripts/jax_train.py:164 dreamer_v3_critic, scripts/jax_policy.py:369
 * DreamerV3Critic).  The reference's own arithmetic lives in madrona_learn, which is not part of its tree; this contract
 * is the project's own, after Hafner et al. 2023 (DreamerV3, first version: the expectation is taken in symlog space and
 * then decoded).  Over n samples (n is free, as for hs_ppo_loss) one kernel (csrc/hs_k_twohot.h) reads the B logits of a
 * sample once and writes the decoded value and, with returns, the gradient of the cross-entropy against the two-hot
 * target and the sums behind the value statistics.  Without returns the call is the rollout's decode.
 * The arithmetic is the contract.  Narrow logits are widened to f32 exactly; everything is IEEE f32, unfused, in exactly
 * this order; expf / logf / expm1f / log1pf are the accurate library functions.  B = bins, l_i the logits of a sample:
 *   step = (hi - lo) / (float)(B - 1);       b_i = lo + (float)i * step
 *   m = max_i l_i;   d_i = l_i - m;   e_i = expf(d_i)
 *   S = sum_i e_i;   Y = sum_i (e_i * b_i)      both in this order: lane h of 8 adds its bins h, h + 8, h + 16, ... in
 *                                               ascending order onto 0; the 8 partials p_h are combined as
 *                                               ((p_0 + p_1) + (p_2 + p_3)) + ((p_4 + p_5) + (p_6 + p_7))
 *   rS = 1.0f / S;   y = Y * rS;      v = copysignf(expm1f(fabsf(y)), y)                  the decoded value
 * and with returns R:
 *   z  = copysignf(log1pf(fabsf(R)), R);   zc = fminf(fmaxf(z, lo), hi)                   (R = +-inf lands on hi / lo)
 *   u  = (zc - lo) / step;   k = min(max((int)floorf(u), 0), B - 2);   f = fminf(fmaxf(u - (float)k, 0), 1)
 *   logS = logf(S);   lp_j = d_j - logS
 *   ce = -((1.0f - f) * lp_k + f * lp_{k+1})
 *   p_i = e_i * rS;   t_k = 1.0f - f;   t_{k+1} = f;   t_i = 0 elsewhere
 *   active = mask == null || mask != 0;   cnt = the number of active samples (counted on the device before; the
 *   normaliser of hs_ppo_loss, so the two calls' gradients add);   w = grad_scale / (float)cnt
 *   g_i = w * (loss_coef * (p_i - t_i));      grad_logits_i = (active && g_i != 0) ? g_i : +0
 *   value = (active && v != 0) ? v : +0
 * These are selects: an inactive sample gets +0 in value and in every grad_logits_i whatever bytes it holds (a NaN
 * there reaches no output) and enters no statistic; a zero of either sign is stored as +0.  An ACTIVE sample must hold
 * finite logits and a return that is not NaN: nothing checks that on the device, and the sample's outputs and the
 * statistics are unspecified otherwise.  The same bits come out on every call, at every position of the sample in the
 * batch, and whichever path (16-byte or element accesses) its bytes take.  value is rounded to value_dtype and
 * grad_logits to grad_dtype to nearest even; only columns 0 .. B-1 of a row of grad_stride elements are written.  With
 * cnt == 0 every output is +0.
 * stats [HS_TWOHOT_STATS] f64, sums over the active samples in f64 of the f32 per-sample values: [0] = sum ce,
 * [1] = sum ((double)v - (double)R)^2, [2] = sum v, [3] = sum R, [4] = sum (double)R^2, [5] = cnt.  Summed without
 * atomics in an order that depends on n alone.  The gradients are those of loss = grad_scale * loss_coef * stats[0] / cnt
 * (loss_coef is the value_loss_coef of the reference's learner).
 * The count and the partial sums go through a workspace of the handle: two calls on one handle must not overlap (a
 * call of hs_ppo_loss may: the workspaces are separate).  value, grad_logits and stats may each be null, not all three;
 * only what is requested is written.  Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing
 * written, hs_last_error says which): a null request or null logits; every output null; grad_logits or stats without
 * returns; an unknown dtype; bins outside [2, HS_TWOHOT_MAX_BINS]; a stride below bins; lo, hi, loss_coef or grad_scale
 * not finite, or lo >= hi; n < 1 or n * stride >= 2^31; a pointer not aligned to its element size (stats: 8 bytes); an
 * output range that overlaps an input range or another output; a call before hs_init or inside an open step.  It reads
 * no export and writes no simulator state.  hs_twohot_value is ordered after the device's legacy default stream and
 * blocking; hs_twohot_value_async enqueues on the caller's hipStream_t without synchronising. */
enum { HS_TWOHOT_STATS = 6, HS_TWOHOT_MAX_BINS = 256 };
typedef struct hs_twohot_request {
    const void    *logits;        /* [n][logits_stride] of logits_dtype: the critic's logits over the bins */
    const float   *returns;       /* [n] f32, or null = decode only (value alone may then be requested) */
    const float   *mask;          /* [n] f32 (self_mask: 1.0 / 0.0), or null = all active */
    int32_t n;                    /* samples, n >= 1 and n * stride < 2^31 */
    int32_t logits_dtype;         /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t logits_stride;        /* elements, >= bins */
    int32_t bins;                 /* B in [2, HS_TWOHOT_MAX_BINS]; 255 in the reference's configuration */
    float lo, hi;                 /* the first and the last bin in symlog space, finite, lo < hi; -20, 20 */
    float loss_coef, grad_scale;  /* finite */
    int32_t value_dtype;          /* of value */
    int32_t grad_dtype;           /* of grad_logits */
    int32_t grad_stride;          /* elements, >= bins */
    int32_t reserved;             /* ignored */
    void   *value;                /* [n] of value_dtype, or null */
    void   *grad_logits;          /* [n][grad_stride] of grad_dtype, or null */
    double *stats;                /* [HS_TWOHOT_STATS] f64, or null */
} hs_twohot_request;              /* 96 bytes */
int32_t hs_twohot_value(hs_sim *sim, const hs_twohot_request *req);
int32_t hs_twohot_value_async(hs_sim *sim, void *hip_stream, const hs_twohot_request *req);

/* The entity encoder: the first layer of the reference's SimpleNet (scripts/jax_policy.py:113-161, the network
 * make_policy selects with use_simple=True) over rows of hs_pack_policy_inputs.  Every entity of the four tables
 *   g = 0 self (K = 45 columns, 1 entity), 1 agents (K = 14, 5), 2 boxes (K = 17, 9), 3 ramps (K = 14, 2)
 * (columns 0, 45, 115 and 268 of the row onwards, entity j of a table at its first column + j K) goes through the
 * table's own Dense(E), a LayerNorm and a leaky ReLU; agents, boxes and ramps are max-pooled over their entities; the
 * results are written side by side as features [n][4 E] in the order self | agents | boxes | ramps.  One kernel
 * (csrc/hs_k_embed.h) reads a row once and writes its features; n is free, as for hs_ppo_loss.
 * params is one array of HS_EMBED_PARAM_ROWS * E f32: for each table in the order above W_g [K_g][E] (in-features
 * major), then b_g [E], gamma_g [E], beta_g [E]; the tables' blocks start at rows 0, 48, 65 and 85 of E floats.
 * The arithmetic is the contract.  Narrow rows are widened to f32 exactly; everything is IEEE f32, unfused except
 * where fmaf is written, in exactly this order.  For entity j of table g with inputs x_0 .. x_{K-1} and channel c < E:
 *   z_c = b_g[c];   z_c = fmaf(x_k, W_g[k][c], z_c)   for k = 0, 1, ..., K - 1
 *   sum_c(p): lane l < L = min(E, 64) starts from p_l and, at E = 128, adds p_{l+64}; then for m = 1, 2, 4, ..., L / 2
 *             every lane replaces its value s_l by s_l + s_{l xor m} (a butterfly: every lane ends with the same bits)
 *   mu = sum_c(z_c) / (float)E;   d_c = z_c - mu;   var = sum_c(d_c * d_c) / (float)E
 *   rstd = 1.0f / sqrtf(var + eps)                                  (division and sqrtf correctly rounded)
 *   zhat_c = d_c * rstd;   y_c = fmaf(zhat_c, gamma_g[c], beta_g[c])
 *   a_c = y_c >= 0 ? y_c : slope * y_c
 *   features[row][g E + c] = max_j a_c(j);   argmax[row][g - 1][c] = the LOWEST j that attains it (g >= 1)
 * and for the self table features = a_c.  features is rounded to features_dtype to nearest even.  eps = 1e-6 and
 * slope = 0.01 are flax's defaults; the reference's LayerNorm comes from madrona_learn, which is not part of its tree,
 * so its constants are not pinned by it.
 * Ties: an exact tie goes to the first entity, where JAX's gradient of max splits it evenly.  Apart from coincidences
 * entities tie because their inputs are identical (the actor's masked-out entities are all-zero rows), and for
 * identical inputs the gradient of every parameter is the same under either rule.
 * hs_entity_encode_backward takes the same rows and parameters, the upstream grad_features [n][4 E] and the forward's
 * argmax, recomputes z, mu, rstd, zhat and y as above (nothing but argmax is saved) and writes grad_params
 * [HS_EMBED_PARAM_ROWS * E] f32 in the layout of params.  No gradient with respect to the rows is computed:
 * observations are leaves and the normaliser is not trained by gradient.  Per entity j of table g:
 *   dy_c = (g == 0 || argmax_c == j) ? grad_features_c * (y_c >= 0 ? 1.0f : slope) : 0
 *   h_c = gamma_c * dy_c;   mh = sum_c(h_c) / (float)E;   mhz = sum_c(h_c * zhat_c) / (float)E
 *   dz_c = rstd * ((h_c - mh) - zhat_c * mhz)
 *   dW[k][c] = fmaf(x_k, dz_c, dW[k][c]);   db_c = db_c + dz_c;   dgamma_c = fmaf(dy_c, zhat_c, dgamma_c);
 *   dbeta_c = dbeta_c + dy_c
 * An entity that no channel selected adds nothing and may be skipped.  The sums over the rows run in an order that
 * depends on n and E alone: with R = HS_EMBED_ROWS_PER_WAVE(E) * 4 rows per round and G = min(ceil(n / R),
 * HS_EMBED_MAX_GRID_BWD) workgroups, workgroup b takes rounds b, b + G, ...; wave w of it the rows
 * round * R + w * R / 4 + s (s < R / 4); a lane adds its rows' terms in round order onto +0 and the entities of a row in
 * ascending j; at E = 32 the halves s = 0, 1 are added as (s0 + s1); the waves as ((w0 + w1) + w2) + w3; the workgroups'
 * sums go to a workspace of the handle, where HS_EMBED_SUM_SEGS segments of ceil(G / segs) consecutive workgroups are
 * each added in ascending order onto +0 and the segments then in ascending order.  No atomics: the same inputs give the
 * same bits on every call, and a row's features do not depend on its position, on n or on the path (16-byte or element
 * loads) its bytes take.  grad_features all +0 gives grad_params all +0.
 * Rows, parameters and upstream gradients must be finite: nothing checks that on the device.
 * Two backward calls on one handle must not overlap (the workspace); forward calls may.  Everything is validated
 * before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a null request, null
 * rows or params, every output null (backward: a null grad_features, argmax or grad_params); an unknown dtype;
 * embed_dim not 32, 64 or 128; n < 1 or n * 296 or n * 4 E >= 2^31; eps or slope not finite, or eps <= 0; a pointer not
 * aligned to its element size (params and grad_params: 4 bytes); an output range that overlaps an input range or
 * another output; a call before hs_init or inside an open step.  The calls read no export and write no simulator
 * state.  The blocking forms are ordered after the device's legacy default stream; the _async forms enqueue on the
 * caller's hipStream_t without synchronising. */
enum { HS_EMBED_PARAM_ROWS = 102, HS_EMBED_MAX_GRID_BWD = 512, HS_EMBED_SUM_SEGS = 8 };
#define HS_EMBED_ROWS_PER_WAVE(E) ((E) == 32 ? 2 : 1)
typedef struct hs_entity_encode_request {
    const void    *rows;          /* [n][HS_PACK_ROW] of rows_dtype, contiguous */
    const float   *params;        /* [HS_EMBED_PARAM_ROWS * embed_dim] f32 */
    int32_t n;                    /* rows, n >= 1 */
    int32_t rows_dtype;           /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t embed_dim;            /* E: 32, 64 (the reference's) or 128 */
    int32_t features_dtype;       /* of features */
    float eps, slope;             /* finite, eps > 0; 1e-6, 0.01 */
    void    *features;            /* [n][4 E] of features_dtype, or null */
    uint8_t *argmax;              /* [n][3][E]: agents, boxes, ramps; or null */
} hs_entity_encode_request;       /* 56 bytes */
typedef struct hs_entity_encode_backward_request {
    const void    *rows;          /* as in the forward call */
    const float   *params;
    const void    *grad_features; /* [n][4 E] of grad_dtype */
    const uint8_t *argmax;        /* [n][3][E], what the forward call wrote */
    int32_t n;
    int32_t rows_dtype;
    int32_t embed_dim;
    int32_t grad_dtype;           /* of grad_features: HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    float eps, slope;
    float   *grad_params;         /* [HS_EMBED_PARAM_ROWS * embed_dim] f32 */
} hs_entity_encode_backward_request;  /* 64 bytes */
int32_t hs_entity_encode(hs_sim *sim, const hs_entity_encode_request *req);
int32_t hs_entity_encode_async(hs_sim *sim, void *hip_stream, const hs_entity_encode_request *req);
int32_t hs_entity_encode_backward(hs_sim *sim, const hs_entity_encode_backward_request *req);
int32_t hs_entity_encode_backward_async(hs_sim *sim, void *hip_stream, const hs_entity_encode_backward_request *req);

/* The recurrent core: what the reference's PolicyRNN (scripts/jax_policy.py, make_policy: an LSTM of 256 hidden channels
 * and one layer, a LayerNorm on its output, clear_recurrent_state at episode ends) does after its two gate GEMMs.  The
 * caller computes gates [n][4 H] = x W_in + h_prev W_rec with the BLAS library; one kernel (csrc/hs_k_lstm.h) then reads
 * a row's 4 H gate values and H cell values once and writes y, h_next and c_next; n is free, as for hs_ppo_loss.
 * madrona_learn's LSTM, LayerNorm and clear_recurrent_state are not part of the reference's tree: the gate order, the
 * eps and the place of the clear below are the project's own and are not pinned by it.
 * cell_params is one array of HS_LSTM_PARAM_ROWS * H f32: bias [4 H] | gamma [H] | beta [H].  The gate k of channel c
 * is gates[r][k H + c] and bias[k H + c], in the order k = 0 i (input), 1 f (forget), 2 g (candidate), 3 o (output).
 * The arithmetic is the contract.  Narrow gates are widened to f32 exactly; everything is IEEE f32, unfused except
 * where fmaf is written, in exactly this order; expf and tanhf are the device library's accurate functions and are not
 * pinned bit for bit.  For row r and channel c < H:
 *   zi = gates_i + bias_i;   zf = gates_f + bias_f;   zg = gates_g + bias_g;   zo = gates_o + bias_o
 *   sigma(x) = 1.0f / (1.0f + expf(-x))
 *   i = sigma(zi);   f = sigma(zf);   g = tanhf(zg);   o = sigma(zo)
 *   c' = fmaf(f, c_prev, i * g);   tc = tanhf(c');   h' = o * tc
 *   sum_c(p): lane l < 64 adds p_l, p_{l+64}, ..., p_{l+H-64} in ascending order; then for m = 1, 2, 4, ..., 32 every
 *             lane replaces its value s_l by s_l + s_{l xor m} (the butterfly of hs_entity_encode with L = 64: every
 *             lane ends with the same bits)
 *   mu = sum_c(h') / (float)H;   d = h' - mu;   var = sum_c(d * d) / (float)H
 *   rstd = 1.0f / sqrtf(var + eps)                                  (division and sqrtf correctly rounded)
 *   hhat = d * rstd;   y = fmaf(hhat, gamma, beta)
 *   keep = clear == null || clear[r] == 0
 *   y[r][c] = y;   h_next[r][c] = keep ? h' : +0;   c_next[r][c] = keep ? c' : +0           (selects, not products)
 * clear [n] i32 is the done export of the step just taken (as hs_gae_request's done).  y is the LayerNorm of the
 * UNCLEARED h': the reference's PolicyRNN.__call__ norms the LSTM's output, and the clear applies to the carried state
 * alone.  gates is f32, bf16 or f16; c_prev and c_next are always f32; h_next has the dtype of gates (it feeds the next
 * GEMM) and y its own y_dtype, both rounded to nearest even.  y, h_next and c_next may each be null, not all three; only
 * what is requested is written.  A row's outputs do not depend on its position or on n.
 * hs_lstm_cell_backward recomputes all of the above from gates, c_prev, cell_params and clear (nothing else is saved)
 * and takes grad_y [n][H] of y_dtype, grad_h_next [n][H] of gates_dtype or null and grad_c_next [n][H] f32 or null; a
 * null gradient counts as +0.  No gradient with respect to clear exists.
 *   dy = grad_y;   hb = gamma * dy;   mh = sum_c(hb) / (float)H;   mhz = sum_c(hb * hhat) / (float)H
 *   dh = rstd * ((hb - mh) - hhat * mhz) + (keep ? grad_h_next : 0)
 *   dc = fmaf(dh * o, 1.0f - tc * tc, keep ? grad_c_next : 0)
 *   dzo = (dh * tc) * (o * (1.0f - o));          dzi = (dc * g) * (i * (1.0f - i))
 *   dzf = (dc * c_prev) * (f * (1.0f - f));      dzg = (dc * i) * (1.0f - g * g)
 *   grad_gates[r][k H + c] = dz_k   (rounded to gates_dtype);     grad_c_prev[r][c] = dc * f
 *   dbias_k[c] = dbias_k[c] + dz_k;   dgamma[c] = fmaf(dy, hhat, dgamma[c]);   dbeta[c] = dbeta[c] + dy
 * grad_cell_params [HS_LSTM_PARAM_ROWS * H] f32 has the layout of cell_params.  Its sums over the rows run in an order
 * that depends on n alone: with R = HS_LSTM_ROWS_PER_ROUND rows per round and G = min(ceil(n / R), HS_LSTM_MAX_GRID_BWD)
 * workgroups, workgroup b takes rounds b, b + G, ...; wave w of it row round * R + w; a lane adds its rows' terms in
 * round order onto +0; the waves add as ((w0 + w1) + w2) + w3; the workgroups' sums go to a workspace of the handle
 * ([HS_LSTM_MAX_GRID_BWD][HS_LSTM_PARAM_ROWS * HS_LSTM_MAX_HIDDEN] f32), where HS_EMBED_SUM_SEGS segments of
 * ceil(G / segs) consecutive workgroups are each added in ascending order onto +0 and the segments then in ascending
 * order (the kernel that does so is hs_entity_encode_backward's).  Rows past n contribute nothing.  No atomics: the same
 * inputs give the same bits on every call.  All-zero gradients give grad_cell_params all +0 (and grad_gates and
 * grad_c_prev zeros of either sign).  grad_gates, grad_c_prev and grad_cell_params may each be null, not all three.
 * Gates, cell values, parameters and gradients must be finite: nothing checks that on the device.
 * Two backward calls on one handle must not overlap (the workspace); forward calls may.  Everything is validated
 * before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a null request, null
 * gates, c_prev or cell_params, every output null (backward: also a null grad_y); an unknown dtype; hidden not 64, 128,
 * 256 or 512; n < 1 or n * 4 H >= 2^31; eps not finite or <= 0; a pointer not aligned to its element size (f32 and i32
 * arrays: 4 bytes); an output range that overlaps an input range or another output; a call before hs_init or inside an
 * open step.  The calls read no export and write no simulator state.  The blocking forms are ordered after the device's
 * legacy default stream; the _async forms enqueue on the caller's hipStream_t without synchronising. */
enum { HS_LSTM_PARAM_ROWS = 6, HS_LSTM_MAX_GRID_BWD = 512, HS_LSTM_MAX_HIDDEN = 512, HS_LSTM_ROWS_PER_ROUND = 4 };
typedef struct hs_lstm_cell_request {
    const void    *gates;         /* [n][4 hidden] of gates_dtype, contiguous: i | f | g | o */
    const float   *c_prev;        /* [n][hidden] f32 */
    const float   *cell_params;   /* [HS_LSTM_PARAM_ROWS * hidden] f32: bias [4 H] | gamma [H] | beta [H] */
    const int32_t *clear;         /* [n] i32 (the done export: nonzero = the episode ended), or null = keep every row */
    int32_t n;                    /* rows, n >= 1 and n * 4 * hidden < 2^31 */
    int32_t hidden;               /* H: 64, 128, 256 (the reference's) or 512 */
    int32_t gates_dtype;          /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16; of gates and h_next */
    int32_t y_dtype;              /* of y */
    float eps;                    /* finite, > 0; 1e-6 */
    int32_t reserved;             /* ignored */
    void    *y;                   /* [n][hidden] of y_dtype, or null */
    void    *h_next;              /* [n][hidden] of gates_dtype, or null */
    float   *c_next;              /* [n][hidden] f32, or null */
} hs_lstm_cell_request;           /* 80 bytes */
typedef struct hs_lstm_cell_backward_request {
    const void    *gates;         /* as in the forward call */
    const float   *c_prev;
    const float   *cell_params;
    const int32_t *clear;
    const void    *grad_y;        /* [n][hidden] of y_dtype */
    const void    *grad_h_next;   /* [n][hidden] of gates_dtype, or null = +0 */
    const float   *grad_c_next;   /* [n][hidden] f32, or null = +0 */
    int32_t n;
    int32_t hidden;
    int32_t gates_dtype;          /* of gates, grad_h_next and grad_gates */
    int32_t y_dtype;              /* of grad_y */
    float eps;
    int32_t reserved;             /* ignored */
    void    *grad_gates;          /* [n][4 hidden] of gates_dtype, or null */
    float   *grad_c_prev;         /* [n][hidden] f32, or null */
    float   *grad_cell_params;    /* [HS_LSTM_PARAM_ROWS * hidden] f32, or null */
} hs_lstm_cell_backward_request;  /* 104 bytes */
int32_t hs_lstm_cell(hs_sim *sim, const hs_lstm_cell_request *req);
int32_t hs_lstm_cell_async(hs_sim *sim, void *hip_stream, const hs_lstm_cell_request *req);
int32_t hs_lstm_cell_backward(hs_sim *sim, const hs_lstm_cell_backward_request *req);
int32_t hs_lstm_cell_backward_async(hs_sim *sim, void *hip_stream, const hs_lstm_cell_backward_request *req);

/* A dense layer after its GEMM: what one layer of the reference's MLP(num_channels=256, num_layers=3) at the end of
 * SimpleNet (scripts/jax_policy.py:163-167) does to the GEMM's result, Dense -> LayerNorm -> leaky ReLU, the order
 * SimpleNet.embed shows.  The caller computes z [n][C] = x W with the BLAS library, WITHOUT the bias; one kernel
 * (csrc/hs_k_dense.h) then reads a row's C values once and writes y; n is free, as for hs_lstm_cell.  madrona_learn's MLP
 * and LayerNorm are not part of the reference's tree: eps = 1e-6 and slope = 0.01 are flax's defaults and
 * hs_entity_encode's, and are not pinned by it.
 * params is one array of HS_DENSE_PARAM_ROWS * C f32: bias [C] | gamma [C] | beta [C].
 * The arithmetic is the contract.  A narrow z is widened to f32 exactly; everything is IEEE f32, unfused except where
 * fmaf is written, in exactly this order.  For row r and channel c < C:
 *   a_c = z_c + bias_c
 *   sum_c(p): with V = C / 64, lane l < 64 holds the ADJACENT channels V l, ..., V l + V - 1 and adds p_{V l}, p_{V l + 1},
 *             ..., p_{V l + V - 1} in ascending order; then for m = 1, 2, 4, ..., 32 every lane replaces its value s_l by
 *             s_l + s_{l xor m} (a butterfly: every lane ends with the same bits).  This order is this call's own: it is
 *             not hs_lstm_cell's, whose lane l holds the channels l, l + 64, ...
 *   mu = sum_c(a_c) / (float)C;   d_c = a_c - mu;   var = sum_c(d_c * d_c) / (float)C
 *   rstd = 1.0f / sqrtf(var + eps)                                  (division and sqrtf correctly rounded)
 *   h_c = d_c * rstd;   u_c = fmaf(gamma_c, h_c, beta_c)
 *   y[r][c] = u_c > 0 ? u_c : slope * u_c                           (rounded to y_dtype to nearest even)
 * The LayerNorm is hs_entity_encode's and hs_lstm_cell's expression.  u_c == 0 takes the slope branch here and in the
 * backward (torch's convention).  A row's y does not depend on its position or on n.
 * hs_dense_norm_act_backward recomputes all of the above from z and params (nothing else is saved) and takes grad_y
 * [n][C] of y_dtype:
 *   g_c = grad_y[r][c];   du_c = u_c > 0 ? g_c : slope * g_c
 *   dh_c = du_c * gamma_c;   m1 = sum_c(dh_c) / (float)C;   m2 = sum_c(dh_c * h_c) / (float)C
 *   da_c = rstd * ((dh_c - m1) - h_c * m2);   grad_z[r][c] = da_c   (rounded to z_dtype)
 *   dbias_c = dbias_c + da_c;   dgamma_c = fmaf(du_c, h_c, dgamma_c);   dbeta_c = dbeta_c + du_c
 * grad_params [HS_DENSE_PARAM_ROWS * C] f32 has the layout of params.  Its sums over the rows run in an order that
 * depends on n alone: with R = HS_DENSE_ROWS_PER_ROUND rows per round and G = min(ceil(n / R), HS_DENSE_MAX_GRID_BWD)
 * workgroups, workgroup b takes rounds b, b + G, ...; wave w of it row round * R + w; a lane adds its rows' terms in
 * round order onto +0; the waves add as ((w0 + w1) + w2) + w3; the workgroups' sums go to a workspace of the handle
 * ([HS_DENSE_MAX_GRID_BWD][HS_DENSE_PARAM_ROWS * HS_DENSE_MAX_CHANNELS] f32, this call's own), where HS_EMBED_SUM_SEGS
 * segments of ceil(G / segs) consecutive workgroups are each added in ascending order onto +0 and the segments then in
 * ascending order (the kernel that does so is hs_entity_encode_backward's).  Rows past n contribute nothing.  No
 * atomics: the same inputs give the same bits on every call.  An all-zero grad_y gives grad_params all +0 (and grad_z
 * zeros of either sign).  grad_z and grad_params may each be null, not both; only what is requested is written.
 * z, parameters and gradients must be finite: nothing checks that on the device.
 * A lane reads and writes its V adjacent elements of a row as one piece of up to 16 bytes, so z, y, grad_y and grad_z
 * must be 16-byte aligned: any contiguous [n][C] array that starts at a row boundary of a 16-byte aligned allocation
 * is.  There is no by-element path for other pointers: they are refused.
 * Two backward calls on one handle must not overlap (the workspace); forward calls may.  Everything is validated
 * before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a null request, null z,
 * params or y (backward: null grad_y, or grad_z and grad_params both null); an unknown dtype; channels not 64, 128, 256
 * or 512; n < 1 or n * C >= 2^31; eps not finite or <= 0; slope not finite or outside [0, 1]; z, y, grad_y or grad_z
 * not 16-byte aligned, params or grad_params not 4-byte aligned; an output range that overlaps an input range or
 * another output; a call before hs_init or inside an open step.  The calls read no export and write no simulator
 * state.  The blocking forms are ordered after the device's legacy default stream; the _async forms enqueue on the
 * caller's hipStream_t without synchronising. */
enum { HS_DENSE_PARAM_ROWS = 3, HS_DENSE_MAX_GRID_BWD = 512, HS_DENSE_MAX_CHANNELS = 512, HS_DENSE_ROWS_PER_ROUND = 4 };
typedef struct hs_dense_norm_act_request {
    const void    *z;             /* [n][channels] of z_dtype, contiguous, 16-byte aligned: x W without the bias */
    const float   *params;        /* [HS_DENSE_PARAM_ROWS * channels] f32: bias [C] | gamma [C] | beta [C] */
    int32_t n;                    /* rows, n >= 1 and n * channels < 2^31 */
    int32_t channels;             /* C: 64, 128, 256 (the reference's) or 512 */
    int32_t z_dtype;              /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t y_dtype;              /* of y */
    float eps, slope;             /* finite, eps > 0, 0 <= slope <= 1; 1e-6, 0.01 */
    void    *y;                   /* [n][channels] of y_dtype, 16-byte aligned */
} hs_dense_norm_act_request;      /* 48 bytes */
typedef struct hs_dense_norm_act_backward_request {
    const void    *z;             /* as in the forward call */
    const float   *params;
    const void    *grad_y;        /* [n][channels] of y_dtype, 16-byte aligned */
    int32_t n;
    int32_t channels;
    int32_t z_dtype;              /* of z and grad_z */
    int32_t y_dtype;              /* of grad_y */
    float eps, slope;
    void    *grad_z;              /* [n][channels] of z_dtype, 16-byte aligned, or null */
    float   *grad_params;         /* [HS_DENSE_PARAM_ROWS * channels] f32, or null */
} hs_dense_norm_act_backward_request;  /* 64 bytes */
int32_t hs_dense_norm_act(hs_sim *sim, const hs_dense_norm_act_request *req);
int32_t hs_dense_norm_act_async(hs_sim *sim, void *hip_stream, const hs_dense_norm_act_request *req);
int32_t hs_dense_norm_act_backward(hs_sim *sim, const hs_dense_norm_act_backward_request *req);
int32_t hs_dense_norm_act_backward_async(hs_sim *sim, void *hip_stream, const hs_dense_norm_act_backward_request *req);

/* The optimiser: the clip by the global gradient norm and the Adam step that end every update of the reference's learner
 * (scripts/jax_train.py: lr = 1e-4, max_grad_norm = 5), over ONE flat f32 buffer each of parameters, gradients and the
 * two moments, n elements each (gpu_hideseek.optim.flatten lays a module's parameters out in such a buffer).  Two
 * kernels (csrc/hs_k_adam.h): one leaves partial sums of squares, the other adds them and updates.  madrona_learn's
 * optimiser is not part of the reference's tree: the rule is optax's clip_by_global_norm followed by Adam (AdamW with
 * weight_decay > 0), this project's statement of it, and not pinned by the reference.
 * The arithmetic is the contract.
 * The norm.  The buffer is cut into quads of 4 adjacent floats, quad q = elements 4 q .. 4 q + 3, Q = ceil(n / 4) quads,
 * the last one short when n is no multiple of 4.  With G = min(ceil(Q / 256), HS_ADAM_MAX_GRID) workgroups of 256 lanes,
 * quad q = (trip * G + b) * 256 + lane belongs to lane `lane` of workgroup b in its trip `trip`.  In f64:
 *   a lane adds (double)g * (double)g (exact) of its elements onto +0, its quads in trip order and a quad's elements in
 *   index order;  a workgroup's partial is ((lane_0 + lane_1) + lane_2) + ... + lane_255;
 *   sum = ((partial_0 + partial_1) + ...) + partial_{G-1}     (every workgroup of the update adds them itself: same bits)
 *   gnorm = grad_scale * sqrt(sum);   skipped = gnorm is not finite        (sqrt and the divisions correctly rounded)
 *   clip = skipped ? 0 : (max_grad_norm > 0 && gnorm > max_grad_norm) ? max_grad_norm / gnorm : 1      (optax's form)
 *   s = (float)(grad_scale * clip)                                       rounded once
 * (grad_scale and max_grad_norm are f64 in the request; a norm that is finite in the gradients' own scale can still
 * overflow through grad_scale, and is then skipped).  No atomics: the same inputs give the same bits on every call.
 * The state, f64 [HS_ADAM_STATE] on the device, = {beta1^t, beta2^t, t, the number of skipped steps}; a fresh one is
 * {1, 1, 0, 0}.  A step that is not skipped multiplies the products by (double)beta1 and (double)beta2, adds 1 to t, and
 *   bc1 = (float)(1 - beta1^t);   bc2 = (float)(1 - beta2^t)             with the new products: no pow
 * Then per element, in IEEE f32, unfused, in exactly this order, with omb1 = (float)(1 - (double)beta1) and
 * omb2 = (float)(1 - (double)beta2) rounded once on the host:
 *   g = g_raw * s
 *   m = beta1 * m + omb1 * g
 *   v = beta2 * v + omb2 * (g * g)
 *   u = (m / bc1) / (sqrtf(v / bc2) + eps)                               (division and sqrtf correctly rounded)
 *   p = p - lr * (u + weight_decay * p)          weight_decay == 0:  p = p - lr * u  (the term is left out, not added as 0)
 * An element's result does not depend on its position or on n, given s, bc1 and bc2.  An element with p = g = m = v = +0
 * stays +0 in p, m and v and adds nothing to the norm: padding between parameters is inert.
 * A skipped step (a NaN or an infinity among the gradients, or a norm that overflows) leaves params, m, v, beta1^t, beta2^t
 * and t exactly as they were; only state[3] grows by 1.  With zero_grad != 0 every element of grads is overwritten with
 * +0, on a skipped step too; with zero_grad == 0 grads is not written.
 * stats, f64 [HS_ADAM_STATS] or null, receives {gnorm, clip, skipped ? 1 : 0, t after the call}.
 * The partial sums and a snapshot of the state go through a workspace of the handle: the first kernel copies the state
 * there and the second reads only that copy and writes only the caller's state, so no workgroup can read a state
 * another has already advanced, whatever order they run in.  Two calls on one handle must not overlap.
 * A lane reads and writes a quad as one piece of 16 bytes, so params, grads, m and v must be 16-byte aligned; any n >= 1
 * is accepted, the short quad goes by element and nothing past n is read or written.  Everything is validated before
 * anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a null request, null params,
 * grads, m, v or state; n < 1 or n >= 2^31; params, grads, m or v not 16-byte aligned, state or stats not 8-byte aligned;
 * lr, eps, weight_decay, grad_scale or max_grad_norm not finite; eps <= 0, lr < 0, weight_decay < 0 or grad_scale <= 0; a
 * beta outside [0, 1); two of the arrays overlapping; a call before hs_init or inside an open step.  The call reads no
 * export and writes no simulator state.  hs_adam_step is ordered after the device's legacy default stream and blocking;
 * hs_adam_step_async enqueues on the caller's hipStream_t without synchronising.
 * Not part of this call: a bf16 / f16 shadow copy of the weights (the modules cast their weights inside the autograd
 * graph), and parameters spread over several devices: data-parallel training keeps one replica per shard, reduces the
 * replicas' gradients with hs_reduce_gradients (below) and makes this call on every replica. */
enum { HS_ADAM_MAX_GRID = 256, HS_ADAM_STATE = 4, HS_ADAM_STATS = 4 };
typedef struct hs_adam_request {
    float   *params;              /* [n] f32, 16-byte aligned: updated in place */
    float   *grads;               /* [n] f32, 16-byte aligned: read; overwritten with +0 when zero_grad != 0 */
    float   *m;                   /* [n] f32, 16-byte aligned: the first moment, updated in place */
    float   *v;                   /* [n] f32, 16-byte aligned: the second moment, updated in place */
    int64_t n;                    /* elements, 1 <= n < 2^31 */
    float lr;                     /* finite, >= 0; 1e-4 */
    float beta1, beta2;           /* in [0, 1); 0.9, 0.999 */
    float eps;                    /* finite, > 0; 1e-8 */
    float weight_decay;           /* finite, >= 0; 0 = plain Adam */
    double max_grad_norm;         /* finite; <= 0 = no clipping; 5 */
    double grad_scale;            /* finite, > 0: the gradients are g_raw * grad_scale (1 / loss scale); 1 */
    int32_t zero_grad;            /* != 0: grads is +0 after the call */
    double *state;                /* [HS_ADAM_STATE] f64 on the device: beta1^t, beta2^t, t, skipped steps */
    double *stats;                /* [HS_ADAM_STATS] f64 on the device, or null */
} hs_adam_request;                /* 104 bytes */
int32_t hs_adam_step(hs_sim *sim, const hs_adam_request *req);
int32_t hs_adam_step_async(hs_sim *sim, void *hip_stream, const hs_adam_request *req);

/* The gradient reduction of data-parallel training: every shard's replica has the gradient of the mean loss over its own
 * active samples in a flat f32 buffer of n elements, and dst receives the gradient of the mean over ALL shards' active
 * samples, the buffers weighted by the shards' counts, in one kernel (csrc/hs_k_reduce.h).  Every replica makes the same
 * call on copies of the same buffers and so holds the same bits: there is no broadcast and no collective library.
 * madrona_learn is not part of the reference's tree; the rule is this project's.  The arithmetic is the contract.
 * With c_g = count[g], g < shards:
 *   C = c_0 + c_1 + ...        in f64, in index order, over the shards with c_g != 0
 *   w_g = (float)(c_g / C)     the division correctly rounded, rounded to f32 once
 * A shard with c_g == 0 is left out by a uniform branch: its buffer is not read and not multiplied by 0, so an infinity or
 * a NaN in it does not reach dst.  Per element, in IEEE f32, unfused, over the remaining shards a < ... < g in index order:
 *   acc = w_a * x_a;   acc = acc + w_g * x_g;   dst = acc
 * If every count is 0, dst is +0.  The counts are taken as they are: a NaN count is not 0, so C and every weight are NaN
 * and so is dst, which hs_adam_step then skips; a NaN or an infinity in a counted buffer propagates likewise.  With one
 * shard and c_0 > 0 the weight is exactly 1 and dst is src[0] bit for bit.  An element's result depends on nothing but
 * its `shards` inputs and the counts: not on its position, on n or on the grid.  No atomics: the same inputs give the same
 * bits on every call.  total, f64 [1] or null, receives C.
 * dst may be exactly one src[g], the same address: a lane reads its quad from every source before it writes it.
 * Otherwise dst must be disjoint from every source; a partial overlap is refused.  The sources may overlap each other.
 * A lane reads and writes a quad of 4 floats as one piece of 16 bytes, so every src[g] and dst must be 16-byte aligned;
 * the short last quad goes by element and nothing past n is read or written.  (shards + 1) * 4 n bytes are moved.
 * Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a
 * null request; shards outside [1, HS_REDUCE_MAX_SHARDS]; n < 1 or n >= 2^31; a null dst, count or src[g < shards]; dst or
 * a src[g] not 16-byte aligned, count or total not 8-byte aligned; dst overlapping a src[g] without being it, or being
 * more than one of them; count overlapping dst; total overlapping dst, count or a src[g]; a call before hs_init or inside
 * an open step.  src[g >= shards] is not looked at.  Every pointer is on the handle's device.  The call reads no export
 * and writes no simulator state.  hs_reduce_gradients is ordered after the device's legacy default stream and blocking;
 * hs_reduce_gradients_async enqueues on the caller's hipStream_t without synchronising.
 * Not part of this call: moving the buffers between devices (the caller copies them next to each other first;
 * gpu_hideseek.trainer.ShardedTrainer does), one process per device, RCCL, overlapping the reduction with the backward
 * pass, and a reduce-scatter form for many shards. */
enum { HS_REDUCE_MAX_SHARDS = 16 };
typedef struct hs_grad_reduce_request {
    const float *src[HS_REDUCE_MAX_SHARDS];   /* each [n] f32, 16-byte aligned; the first `shards` are read */
    const double *count;          /* [shards] f64 on the device: each shard's number of active samples */
    float   *dst;                 /* [n] f32, 16-byte aligned; may be one src[g] */
    int64_t n;                    /* elements, 1 <= n < 2^31 */
    int32_t shards;               /* 1 <= shards <= HS_REDUCE_MAX_SHARDS */
    double *total;                /* [1] f64 on the device, or null: receives C */
} hs_grad_reduce_request;         /* 168 bytes */
int32_t hs_reduce_gradients(hs_sim *sim, const hs_grad_reduce_request *req);
int32_t hs_reduce_gradients_async(hs_sim *sim, void *hip_stream, const hs_grad_reduce_request *req);

/* The dynamic loss scale of float16 training: a scale S on the device that hs_ppo_loss_scaled and hs_twohot_value_scaled
 * multiply their gradients by, and that hs_adam_step_scaled divides out again, halves when the gradient norm overflows
 * and doubles after a run of good steps (csrc/hs_k_loss_scale.h).  No call reads the device from the host.  The rule is
 * the published one of torch.cuda.amp.GradScaler and flax's DynamicScale (start 2^16, halve on overflow, double after
 * 2000 good steps); madrona_learn is not part of the reference's tree, so it is this project's statement and not pinned
 * by the reference.  The arithmetic is the contract.
 * The state, f64 [HS_LOSS_SCALE_STATE] on the device, = {S, the good steps since S last changed, the backoffs so far,
 * the growths so far}; a fresh one is {the initial scale, 0, 0, 0}.
 * The loss calls.  S = (float)state[0], one load;   w = (grad_scale * S) / (float)cnt   with the product in f32;
 * everything else is hs_ppo_loss's and hs_twohot_value's arithmetic word for word.  The statistics hold no S: they are
 * the unscaled loss's.  The state is read, never written.  With grad_scale * S a power of two every output has the bits
 * of the unscaled call whose grad_scale is that product.
 * The optimiser.  The norm is hs_adam_step's, the same order and the same partials.  With S the state's value when the
 * call began, in f64:
 *   e = grad_scale / S;   gnorm = e * sqrt(sum);   skipped = gnorm is not finite
 *   clip as hs_adam_step has it;   s = (float)(e * clip)
 * and the update, the Adam state and stats are hs_adam_step's with e where it has grad_scale: stats[0] is the norm of the
 * unscaled gradients.  Then, in f64:
 *   skipped:   S' = max(S * backoff, min_scale);   good' = 0;   backoffs' = backoffs + 1
 *   else:      good' = good + 1;   if good' >= growth_interval:   S' = min(S * growth, max_scale), good' = 0,
 *              growths' = growths + 1;   otherwise S' = S
 * All factors and bounds are powers of two, so S stays one and every product above is exact: gradients multiplied by 2^k
 * with S = 2^k give the bits of hs_adam_step on the original gradients.
 * The first kernel copies the loss-scale state into the handle's workspace next to the Adam state; the second reads only
 * the copies and writes only the caller's states.  A later loss call on the same stream reads the new S.  No atomics.
 * Validation (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): everything the unscaled entry point
 * refuses; a null state or one not 8-byte aligned; growth, backoff, min_scale or max_scale not a power of two (frexp
 * mantissa 0.5) or outside growth >= 1, 0 < backoff <= 1, 0 < min_scale <= max_scale <= 2^126;
 * growth_interval < 1; reserved != 0; a state that overlaps any other array of the request; a call before hs_init or
 * inside an open step.  Blocking and _async forms as for every other entry point.
 * Not part of these calls: overflow in the forward pass (f16 activations that reach infinity give NaN logits, which no
 * gradient scale repairs), a narrow shadow copy of the weights, several devices, a scale per parameter group. */
enum { HS_LOSS_SCALE_STATE = 4 };
typedef struct hs_loss_scale {
    double *state;                /* [HS_LOSS_SCALE_STATE] f64 on the device, 8-byte aligned */
    double growth, backoff;       /* powers of two; growth >= 1, 0 < backoff <= 1; 2, 0.5 */
    double min_scale, max_scale;  /* powers of two, 0 < min_scale <= max_scale <= 2^126; 1, 2^24 */
    int32_t growth_interval;      /* >= 1; 2000 */
    int32_t reserved;             /* must be 0 */
} hs_loss_scale;                  /* 48 bytes */
int32_t hs_ppo_loss_scaled(hs_sim *sim, const hs_ppo_request *req, const double *loss_scale_state);
int32_t hs_ppo_loss_scaled_async(hs_sim *sim, void *hip_stream, const hs_ppo_request *req, const double *loss_scale_state);
int32_t hs_twohot_value_scaled(hs_sim *sim, const hs_twohot_request *req, const double *loss_scale_state);
int32_t hs_twohot_value_scaled_async(hs_sim *sim, void *hip_stream, const hs_twohot_request *req, const double *loss_scale_state);
int32_t hs_adam_step_scaled(hs_sim *sim, const hs_adam_request *req, const hs_loss_scale *scale);
int32_t hs_adam_step_scaled_async(hs_sim *sim, void *hip_stream, const hs_adam_request *req, const hs_loss_scale *scale);

/* The minibatch gather: cutting shuffled sequences out of a rollout for one minibatch of the update, every field of the
 * rollout in one kernel (csrc/hs_k_gather.h).  The reference trains on back-propagation-through-time chunks
 * (scripts/jax_train.py: steps_per_update = 40, num_bptt_chunks = 8, num_mini_batches = 2); madrona_learn's own gather is
 * not part of the reference's tree, so the layout below is the project's.
 * A rollout of K = chunks chunks of L = chunk_steps steps over n = rows agent rows has K n sequences; sequence id
 * s = k n + r is chunk k of row r.  index [m] i32 on the device holds the ids of a minibatch (a slice of a permutation
 * drawn on the device: nothing here needs the host to know them).  Up to HS_GATHER_MAX_FIELDS fields per call, each
 * {src, dst, row_bytes, per_chunk}:
 *   per_chunk == 0 (a per-step field):   src [K L][n][row_bytes],  dst [L][m][row_bytes]
 *       dst[t][j] = src[k_j L + t][r_j]        for t < L, j < m, with s_j = index[j], k_j = s_j / n, r_j = s_j % n
 *   per_chunk != 0 (a per-chunk field):  src [K][n][row_bytes],    dst [m][row_bytes]
 *       dst[j] = src[k_j][r_j]                 (the LSTM states at the chunks' starts)
 * A pure copy: the bytes of a row arrive unchanged whatever type they hold.  row_bytes is a multiple of 4 and src and dst
 * are 4-byte aligned; a field whose row_bytes is a multiple of 16 and whose src and dst are both 16-byte aligned moves as
 * 16-byte accesses (rows of 592, 512 and 1024 bytes), any other as dwords (rows of 4 and 20 bytes).  Byte offsets are
 * 64-bit: a source may be larger than 2^31 bytes.
 * The kernel never reads outside a source: an id outside [0, K n) leaves zeros in its destination rows of every field,
 * and bad [1] i32, when given, receives the number of such ids among the m (it is zeroed by the call first).  Repeated
 * ids are allowed.  No output may overlap an input or another output.
 * Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a
 * null request or index; m, chunks, chunk_steps or rows below 1; chunks * rows or (num_fields + 1) * m at or above 2^31;
 * num_fields outside [1, HS_GATHER_MAX_FIELDS]; a field with a null src or dst, a row_bytes below 4, above
 * HS_GATHER_MAX_ROW_BYTES or no multiple of 4, or a pointer not 4-byte aligned; index or bad not 4-byte aligned; a dst or
 * bad that overlaps a src, index or another output; a call before hs_init or inside an open step.  The sizes of the
 * sources cannot be checked here: the caller vouches that each holds the rows stated above.  The call reads no export and
 * writes no simulator state.  hs_gather_sequences is ordered after the device's legacy default stream and blocking;
 * hs_gather_sequences_async enqueues on the caller's hipStream_t without synchronising. */
enum { HS_GATHER_MAX_FIELDS = 16, HS_GATHER_MAX_ROW_BYTES = 1048576 };
typedef struct hs_gather_field {
    const void *src;              /* [K L][n][row_bytes] or, per chunk, [K][n][row_bytes]; 4-byte aligned */
    void *dst;                    /* [L][m][row_bytes] or, per chunk, [m][row_bytes]; 4-byte aligned */
    int32_t row_bytes;            /* a multiple of 4, 4 .. HS_GATHER_MAX_ROW_BYTES */
    int32_t per_chunk;            /* 0: a row per step; != 0: a row per chunk */
} hs_gather_field;                /* 24 bytes */
typedef struct hs_gather_request {
    const int32_t *index;         /* [m] i32 on the device: sequence ids k * rows + r */
    int32_t m;                    /* sequences of the minibatch, >= 1 */
    int32_t chunks;               /* K >= 1 */
    int32_t chunk_steps;          /* L >= 1 */
    int32_t rows;                 /* n >= 1; chunks * rows < 2^31 */
    int32_t num_fields;           /* 1 .. HS_GATHER_MAX_FIELDS */
    int32_t reserved;
    int32_t *bad;                 /* [1] i32 on the device or null: the number of ids outside [0, chunks * rows) */
    hs_gather_field fields[HS_GATHER_MAX_FIELDS];
} hs_gather_request;              /* 424 bytes */
int32_t hs_gather_sequences(hs_sim *sim, const hs_gather_request *req);
int32_t hs_gather_sequences_async(hs_sim *sim, void *hip_stream, const hs_gather_request *req);

/* Episode statistics: how the game is going.  One call after a step advances a tracker per agent row (row = world * A +
 * slot) and per world, and folds every episode that ended with that step into a table of f64 sums (csrc/hs_k_episode.h:
 * one kernel over the rows, one lane per row, then the fixed-order add of the workgroups' partial sums onto the table).
 * Inputs, each [rows] unless said otherwise, device memory of the handle's GPU; a null pointer means the handle's own:
 *   reward f32, done i32, self_type i32 (0 = seeker, nonzero = hider), self_mask f32: the exports after the step;
 *   episode_result [worlds][2] f32: the export; hider_team [worlds] i32: the team index (0 or 1) of the hiders in the
 *   world's CURRENT episode, null = the handle's own team order (1 where the seekers are team 0).
 * State, caller-owned device memory, read and written in place: per row ret, disc, gpow f32 and len, type, phase i32
 * (phase: HS_EPISODE_OUT = 0, HS_EPISODE_TRACKED = 1, HS_EPISODE_WAITING = 2 = waiting for its next episode start);
 * per world world_hider_team and world_phase i32 (0 = no team latched yet, 1 = latched).
 * The arithmetic is the contract: IEEE f32, unfused, in exactly this order.  Per row, with R = reward, m = self_mask:
 *   was = phase == 1
 *   if was:    ret = ret + R;  disc = disc + gpow * R;  gpow = gpow * gamma;  len = len + 1
 *   ended = was && done != 0
 *   if ended:  the side of `type` (the latched one, not this step's self_type: 0 = seekers, nonzero = hiders) gains
 *              1 episode, ret, ret^2, disc, len: each the f64 of the f32 / i32 value, the square taken in f64
 *   restart = done != 0 || (phase != 2 && (!was || m == 0))          (phase as it was before this call)
 *   if restart: ret = disc = +0.0, gpow = 1, len = 0, type = self_type, phase = m != 0 ? 1 : 0
 * A row that was not tracked uses no reward (a select, not a product with zero): a row that is out or waiting adds
 * nothing, whatever stale done or NaN reward it carries.  The observation exported together with done != 0 is the first of
 * the NEXT episode (and so are self_type and self_mask, which HS_FLAG_RANDOM_FLIP_TEAMS and changing team sizes alter):
 * hence the latched type.  `restart` is the rule by which the learner zeroes its recurrent state: a row that joins exports
 * done = 0 and starts at zero, a row that leaves keeps a stale done and goes out; a waiting row starts on a done only.
 * Per world, after its rows: the world ended if any of its rows ended.  Then, with h = world_hider_team (the latched one):
 *   world_episodes gains 1;  if world_phase == 1 and h is 0 or 1, x = episode_result[w][h]:
 *   x == 1.0 hider_wins gains 1, x == 0.0 seeker_wins gains 1, x == 0.5 draws gains 1 (any other x: none of them).
 * Then, if the world ended or any of its rows restarted: world_hider_team = hider_team[w], world_phase = 1.
 * table [HS_EPISODE_STATS] f64, for the seekers [0..4] and then the hiders [5..9]: episodes, sum ret, sum ret^2, sum disc,
 * sum len; then [10] hider_wins, [11] seeker_wins, [12] draws, [13] world_episodes.  A call ADDS this step's sums to the
 * table: zeroing it is the caller's business.  This step's sums are added without atomics, in an order that depends on the
 * handle's (worlds, A) alone, starting from +0.0, and then added to the table once: the same inputs give the same bits on
 * every call.  The partial sums go through a workspace of the handle, so two calls on one handle must not overlap.
 * A reset the host requests in mid-episode sets no done and is not covered: the episode it cuts short runs on into the
 * next one.  Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says
 * which): a null request; a null state pointer or table; gamma not finite or outside [0, 1]; a pointer not aligned to
 * its element size (table: 8 bytes); a state array or the table overlapping an input, another state array or the table; a
 * call before hs_init or inside an open step.  Under HS_FLAG_EXT_SKIP_OBSERVATIONS a null self_type or self_mask is
 * refused with HS_ERR_UNSUPPORTED (the observation stage refreshes them after a reset, and it does not run); with both
 * given the call works there.  Writes no simulator state.  hs_episode_stats is ordered after the device's legacy default
 * stream and blocking; hs_episode_stats_async enqueues on the caller's hipStream_t without synchronising (the caller
 * orders it after the step that wrote the exports). */
enum { HS_EPISODE_STATS = 14, HS_EPISODE_SIDE_STATS = 5 };
enum { HS_EPISODE_OUT = 0, HS_EPISODE_TRACKED = 1, HS_EPISODE_WAITING = 2 };
typedef struct hs_episode_request {
    const float   *reward;        /* [rows] f32 or null = the reward export */
    const int32_t *done;          /* [rows] i32 or null = the done export */
    const int32_t *self_type;     /* [rows] i32 or null = the self_type export */
    const float   *self_mask;     /* [rows] f32 or null = the self_mask export */
    const float   *episode_result;        /* [worlds][2] f32 or null = the episode_result export */
    const int32_t *hider_team;    /* [worlds] i32 or null = the handle's team order */
    float gamma;                  /* finite, in [0, 1] */
    int32_t reserved;
    float   *ret, *disc, *gpow;   /* [rows] f32 each, read and written */
    int32_t *len, *type, *phase;  /* [rows] i32 each, read and written */
    int32_t *world_hider_team, *world_phase;      /* [worlds] i32 each, read and written */
    double  *table;               /* [HS_EPISODE_STATS] f64, added to */
} hs_episode_request;             /* 128 bytes */
int32_t hs_episode_stats(hs_sim *sim, const hs_episode_request *req);
int32_t hs_episode_stats_async(hs_sim *sim, void *hip_stream, const hs_episode_request *req);

/* Behaviour statistics: what the agents do with the level.  One call after a step advances a tracker per world (how far
 * the boxes and ramps have been moved in the preparation phase and in the main phase, which of them each side has locked
 * when the seekers are released and at the end, how far each side travels and how often it grabs) and folds every episode
 * that ended with that step into a table of f64 sums (csrc/hs_k_behaviour.h: one kernel, one lane per world, then the
 * fixed-order add of the workgroups' partial sums onto the table).
 * Inputs, device memory of the handle's GPU; a null pointer means the handle's own:
 *   positions [worlds][17][2] f32: the global_positions export; entries 0-8 are the boxes, 9-10 the ramps, 11-16 the
 *     agents, the hiders first and then the seekers, as globalPositionsDebugSystem writes them;
 *   locks [worlds][11] i32, per box and then per ramp: 0 free, 1 locked by the hiders, 2 locked by the seekers; null = the
 *     handle's body metadata, which is what columns 15 / 16 of box_data and 12 / 13 of ramp_data export (an object the
 *     world's `counts` do not hold is 0);
 *   counts [worlds][4] i32: boxes, ramps, hiders and seekers of the world's CURRENT episode, null = the handle's own; a
 *     value is used clamped: boxes to [0, 9], ramps to [0, 2], hiders to [0, 6], seekers to [0, 6 - hiders];
 *   prep_counter, done, self_type i32 and self_mask f32, each [rows] (row = world * A + slot): the exports after the step;
 *   grabbing f32, row r at grabbing[r * grab_stride]: null = column 12 (isGrabbing) of the self_data export, stride 13;
 *   move_eps f32, finite and >= 0: an object counts as moved if its displacement is above it.
 * What belongs to which episode.  A step resets before it observes, so positions, locks, counts, prep_counter, self_type,
 * self_mask and grabbing of one call all describe the same moment, and when they come with done != 0 that moment is the
 * FIRST of the next episode.  done alone looks back.  A row that left keeps a stale done: a world ENDED only if some row
 * has done != 0 AND was active in the previous call.  was_active [rows] i32 is state for that: after a call it is this
 * call's self_mask != 0.
 * State, caller-owned device memory, read and written in place.  Per world: phase i32 (HS_BEHAVIOUR_UNARMED = 0: the next
 * observation starts an episode; HS_BEHAVIOUR_PREP = 1; HS_BEHAVIOUR_MAIN = 2; HS_BEHAVIOUR_WAITING = 3: waiting for a
 * done, so that no episode is booked of which a part was not seen); n_obj [2] i32 (boxes, ramps) and n_side [2] i32
 * (seekers, hiders), latched at the episode's start; start_pos [11][2], prep_pos [11][2], last_pos [17][2] f32;
 * prep_locks [11], last_locks [11] i32; travel [2] f32, grab [2] i32, agent_steps [2] i32: side 0 is the seekers, side 1
 * the hiders.  Per row: was_active i32.
 * The arithmetic is the contract: IEEE f32, unfused, in exactly this order.  d(a, b) = sqrtf((ax - bx) * (ax - bx) +
 * (ay - by) * (ay - by)): two differences, two products, one sum and a correctly rounded square root, each one f32
 * operation.  Per world and call:
 *   1. ended as above.  p = prep_counter of the world's lowest row with self_mask != 0.  If there is no such row, bad
 *      gains 1 and the call does nothing more for this world but step 2 and step 6.
 *   2. If ended and phase is 1 or 2, the episode is booked from the state as the previous call left it.  For each kind,
 *      boxes j < n_obj[0] (entries j) and ramps j < n_obj[1] (entries 9 + j):
 *        move_prep_j = d(prep_pos_j, start_pos_j), move_main_j = d(last_pos_j, prep_pos_j); if the episode never reached the
 *        main phase (phase == 1): move_prep_j = d(last_pos_j, start_pos_j), move_main_j = +0, and last_locks stand for
 *        prep_locks.
 *      The kind gains: max_j move_prep, max_j move_main (+0 with no object), the number of j with move_prep_j > move_eps
 *      and with move_main_j > move_eps, the numbers of j locked by the hiders and by the seekers in prep_locks and in
 *      last_locks, and n_obj.  Each side gains travel, grab and agent_steps.  world_episodes gains 1, reached_main gains
 *      phase == 2.
 *   3. If ended, or phase == 0, or (phase != 3 and the world RESTARTED: a row with self_mask != 0 that was not active
 *      in the previous call and has done == 0, hs_episode_stats's rule; with changing team sizes this is the only sign),
 *      this observation starts an episode: n_obj and n_side are latched from counts; start_pos = prep_pos =
 *      positions[0..10], last_pos = positions, prep_locks = last_locks = locks; travel = +0, grab = agent_steps = 0;
 *      phase = p > 0 ? 1 : 2.
 *   4. Otherwise, if phase is 1 or 2, the episode goes on: for the hiders i < n_side[1] at entries 11 + i in ascending
 *      order travel[1] = travel[1] + d(positions_i, last_pos_i), for the seekers i < n_side[0] at entries
 *      11 + n_side[1] + i likewise onto travel[0]; last_pos = positions, last_locks = locks; if phase == 1 and p == 0:
 *      prep_pos = positions[0..10], prep_locks = locks, phase = 2.
 *   5. After 3 or 4, per row with self_mask != 0 and side = self_type != 0: agent_steps[side] += 1 and
 *      grab[side] += grabbing != 0.
 *   6. was_active = self_mask != 0, per row.
 * table [HS_BEHAVIOUR_STATS] f64: [0] world_episodes, [1] reached_main, [2] bad; for the boxes from HS_BEHAVIOUR_BOXES and
 * the ramps from HS_BEHAVIOUR_RAMPS the nine sums of step 2 in the order of the HS_BEHAVIOUR_KIND_* offsets; for the
 * seekers from HS_BEHAVIOUR_SEEKERS and the hiders from HS_BEHAVIOUR_HIDERS sum travel, sum grab, sum agent_steps.  A call
 * ADDS this step's sums (each term the f64 of the f32 / i32 value) to the table: zeroing it is the caller's business.
 * They are added without atomics, in an order that depends on the handle's worlds alone, starting from +0.0, and then
 * added to the table once: the same inputs give the same bits on every call.  The partial sums go through a workspace of
 * the handle, so two calls on one handle must not overlap.
 * A reset the host requests in mid-episode sets no done and is not covered: the episode it cuts short runs on into the
 * next one.  Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says
 * which): a null request; a null state pointer or table; move_eps not finite or negative; grab_stride < 1 with grabbing
 * given; a pointer not aligned to its element size (table: 8 bytes); a state array or the table overlapping an input,
 * another state array or the table; a call before hs_init or inside an open step.  Under HS_FLAG_EXT_SKIP_OBSERVATIONS a
 * null positions, prep_counter, self_type, self_mask or grabbing is refused with HS_ERR_UNSUPPORTED (the observation
 * stage writes them, and it does not run); with all of them given the call works there.  Writes no simulator state.
 * hs_behaviour_stats is ordered after the device's legacy default stream and blocking; hs_behaviour_stats_async enqueues
 * on the caller's hipStream_t without synchronising (the caller orders it after the step that wrote the exports). */
enum { HS_BEHAVIOUR_STATS = 27, HS_BEHAVIOUR_KIND_STATS = 9, HS_BEHAVIOUR_SIDE_STATS = 3 };
enum { HS_BEHAVIOUR_UNARMED = 0, HS_BEHAVIOUR_PREP = 1, HS_BEHAVIOUR_MAIN = 2, HS_BEHAVIOUR_WAITING = 3 };
enum { HS_BEHAVIOUR_WORLD_EPISODES = 0, HS_BEHAVIOUR_REACHED_MAIN = 1, HS_BEHAVIOUR_BAD = 2, HS_BEHAVIOUR_BOXES = 3, HS_BEHAVIOUR_RAMPS = 12,
       HS_BEHAVIOUR_SEEKERS = 21, HS_BEHAVIOUR_HIDERS = 24 };
enum { HS_BEHAVIOUR_KIND_MAX_PREP = 0, HS_BEHAVIOUR_KIND_MAX_MAIN = 1, HS_BEHAVIOUR_KIND_MOVED_PREP = 2, HS_BEHAVIOUR_KIND_MOVED_MAIN = 3,
       HS_BEHAVIOUR_KIND_HIDER_LOCKED_PREP = 4, HS_BEHAVIOUR_KIND_SEEKER_LOCKED_PREP = 5, HS_BEHAVIOUR_KIND_HIDER_LOCKED_END = 6,
       HS_BEHAVIOUR_KIND_SEEKER_LOCKED_END = 7, HS_BEHAVIOUR_KIND_OBJECTS = 8 };
enum { HS_BEHAVIOUR_SIDE_TRAVEL = 0, HS_BEHAVIOUR_SIDE_GRAB = 1, HS_BEHAVIOUR_SIDE_AGENT_STEPS = 2 };
typedef struct hs_behaviour_request {
    const float   *positions;     /* [worlds][17][2] f32 or null = the global_positions export */
    const int32_t *locks;         /* [worlds][11] i32 or null = the handle's body metadata */
    const int32_t *counts;        /* [worlds][4] i32 or null = the handle's own */
    const int32_t *prep_counter;  /* [rows] i32 or null = the prep_counter export */
    const int32_t *done;          /* [rows] i32 or null = the done export */
    const int32_t *self_type;     /* [rows] i32 or null = the self_type export */
    const float   *self_mask;     /* [rows] f32 or null = the self_mask export */
    const float   *grabbing;      /* [rows] f32 at stride grab_stride, or null = column 12 of the self_data export */
    int32_t grab_stride;          /* in elements, >= 1 where grabbing is given */
    float move_eps;               /* finite, >= 0 */
    int32_t *phase, *n_obj, *n_side;              /* [worlds], [worlds][2], [worlds][2] i32, read and written */
    float   *start_pos, *prep_pos, *last_pos;     /* [worlds][11][2], [worlds][11][2], [worlds][17][2] f32 */
    int32_t *prep_locks, *last_locks;             /* [worlds][11] i32 each */
    float   *travel;              /* [worlds][2] f32 */
    int32_t *grab, *agent_steps;  /* [worlds][2] i32 each */
    int32_t *was_active;          /* [rows] i32 */
    double  *table;               /* [HS_BEHAVIOUR_STATS] f64, added to */
} hs_behaviour_request;           /* 176 bytes */
int32_t hs_behaviour_stats(hs_sim *sim, const hs_behaviour_request *req);
int32_t hs_behaviour_stats_async(hs_sim *sim, void *hip_stream, const hs_behaviour_request *req);

/* The league: P policies play each other on one simulator, and are rated.  One call after a step routes every agent row
 * (row = world * A + slot) to a policy, ranks it among that policy's rows, books the games that ended with the step in a
 * P x P table and moves the Elo ratings (csrc/hs_k_league.h: one kernel over the rows, one lane per row, then a
 * one-workgroup fold).  madrona_learn's matchmaking is not part of the reference's tree: this contract is the project's.
 * A league is P = num_policies, 1 <= P <= HS_LEAGUE_MAX_POLICIES.  The teams are equal and fixed: A = 2 k agent rows per
 * world, k = team_size hiders and k seekers (the reference asserts num_hiders == num_seekers for the same purpose), and
 * the handle's number of worlds is a multiple of P^2.  R = worlds * A.
 * Schedule: world w always plays pair q = w mod P^2: policy i = q / P the hiders, policy j = q % P the seekers.  Every
 * ordered pair, i == j included, has worlds / P^2 worlds, and every policy owns exactly R / P rows at every step,
 * whatever HS_FLAG_RANDOM_FLIP_TEAMS does to the order of a world's rows: the P forwards have fixed shapes and nothing is
 * read back from the device to size them.  (A drawn or rotating matchup is balanced only while all worlds' episodes stay
 * in step.)
 * Inputs, device memory of the handle's GPU; a null pointer means the handle's own:
 *   done i32, self_type i32 (0 = seeker, nonzero = hider), self_mask f32, each [R]: the exports after the step;
 *   episode_result [worlds][2] f32: the export; hider_team [worlds] i32: the team index (0 or 1) of the hiders in the
 *   world's CURRENT episode, null = the handle's own team order, as hs_episode_stats takes it.
 * Sides: a row is a hider iff its self_type is nonzero: the export after the step, which belongs to the NEXT episode when
 * it comes with done (hs_episode_stats above).  A world is malformed if its rows do not split into k hiders and k seekers
 * or if one of its self_mask values is 0: it takes its rows 0 .. k-1 as hiders and k .. 2k-1 as seekers and adds 1 to
 * bad ([1] i32 or null, written by every call: the malformed worlds of this call).  So everything below is a permutation
 * in every case.
 * Routing outputs, each [R] i32:
 *   policy_assignments[row] = the policy of the row's side; null = the handle's policy_assignments export, which feeds
 *     the simulator as the reference's is fed;
 *   slot[row] = the row's rank in the stable sort of all rows by (policy, row); row_of_slot[slot] = row, its inverse;
 *   clear_slot[slot] = done[row] of the row now at that slot.  slot, row_of_slot and clear_slot may each be null.
 * Slots [p R / P, (p + 1) R / P) are policy p's block.  The rank needs no scan and no sort: with g = w / P^2, policy p's
 * block gets 2 P k slots per group g, starting at p R / P + g 2 P k; the world's offset in them is k times the number of
 * sides p holds in the worlds of the group before q; the rank inside the world is the number of earlier rows of the world
 * with the same policy.  What a caller that keeps state per slot relies on: the SET of slots a world owns does not change
 * when its teams flip (a policy's rows of a world are one run of k, or with i == j of 2 k, slots), and a row changes slot
 * only at an episode start, where recurrent state is zero anyway.
 * Per-world state, caller-owned, read and written in place: world_hider_team i32 and world_phase i32 (0 = nothing
 * latched, 1 = latched), [worlds] each.  With fixed teams a world's rows carry one done: the world ended with this step
 * iff the done of its first row is nonzero.  In this order:
 *   if the world ended and world_phase == 1: h = world_hider_team (the latched one); x = episode_result[w][h];
 *     outcome o = 0 if x == 1.0 (the hiders win), 1 if x == 0.0 (the seekers win), 2 if x == 0.5 (a draw), 3 for any
 *     other x, NaN included, and (without a read) for h outside {0, 1}: played, no outcome.  counts[i][j][o] gains 1.
 *   if the world ended or world_phase == 0: world_hider_team = hider_team[w], world_phase = 1.
 * counts [P][P][HS_LEAGUE_OUTCOMES] i64 is ADDED to (integers: the order of addition cannot show).
 * Elo: elo [P] f64, read and written.  Ratings are batched by step: with D the counts this call added, and elo as it
 * stood BEFORE the call, every ordered pair i != j has
 *   n = D[i][j][0] + D[i][j][1] + D[i][j][2];   S = D[i][j][0] + 0.5 D[i][j][2]
 *   E = 1 / (1 + 10^((elo[j] - elo[i]) / 400));   d = k_factor (S - n E), and d = +0.0 where n == 0 (E is not formed)
 * and then, in ascending (i, j), elo[i] = elo[i] + d and elo[j] = elo[j] - d.  All f64, unfused.  The games that end with
 * one step are all rated against the ratings before it, so their order within the step cannot matter; pairs with i == j
 * and games with o == 3 move nothing; a call in which every d is zero writes no rating.  The same inputs give the same
 * bits on every call.  The step's counts go through a table of the handle, so two calls on one handle must not overlap.
 * Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a
 * null request; null world_hider_team, world_phase, counts or elo; num_policies outside [1, HS_LEAGUE_MAX_POLICIES];
 * team_size < 1 or the handle's A != 2 team_size; worlds not a multiple of P^2; k_factor not finite or not above 0; a
 * pointer not aligned to its element size; an output overlapping an input or another output (the handle's exports
 * included where a null pointer names them); a call before hs_init or inside an open step.  Under
 * HS_FLAG_EXT_SKIP_OBSERVATIONS a null self_type or self_mask is refused with HS_ERR_UNSUPPORTED; with both given the
 * call works there.  Writes no simulator state other than the policy_assignments export when that pointer is null.
 * hs_league_step is ordered after the device's legacy default stream and blocking; hs_league_step_async enqueues on the
 * caller's hipStream_t without synchronising (the caller orders it after the step that wrote the exports). */
enum { HS_LEAGUE_MAX_POLICIES = 16, HS_LEAGUE_OUTCOMES = 4 };
enum { HS_LEAGUE_HIDERS_WIN = 0, HS_LEAGUE_SEEKERS_WIN = 1, HS_LEAGUE_DRAW = 2, HS_LEAGUE_NO_OUTCOME = 3 };
typedef struct hs_league_request {
    const int32_t *done;          /* [R] i32 or null = the done export */
    const int32_t *self_type;     /* [R] i32 or null = the self_type export */
    const float   *self_mask;     /* [R] f32 or null = the self_mask export */
    const float   *episode_result;        /* [worlds][2] f32 or null = the episode_result export */
    const int32_t *hider_team;    /* [worlds] i32 or null = the handle's team order */
    int32_t num_policies;         /* P in [1, HS_LEAGUE_MAX_POLICIES]; worlds % P^2 == 0 */
    int32_t team_size;            /* k >= 1; the handle's A == 2 k */
    double k_factor;              /* finite, > 0 */
    int32_t *policy_assignments;  /* [R] i32 or null = the policy_assignments export */
    int32_t *slot, *row_of_slot, *clear_slot;     /* [R] i32 each, or null */
    int32_t *world_hider_team, *world_phase;      /* [worlds] i32 each, read and written */
    int32_t *bad;                 /* [1] i32 or null: the malformed worlds of this call */
    int64_t *counts;              /* [P][P][HS_LEAGUE_OUTCOMES] i64, added to */
    double  *elo;                 /* [P] f64, read and written */
} hs_league_request;              /* 128 bytes */
int32_t hs_league_step(hs_sim *sim, const hs_league_request *req);
int32_t hs_league_step_async(hs_sim *sim, void *hip_stream, const hs_league_request *req);

/* The league on a schedule read from a table: what a pool of past policies needs (gpu_hideseek.population), where the
 * learners play frozen earlier policies and no world is past against past, which the all-pairs form cannot say.
 * A schedule is `pairs`, G = group pairs (hider policy, seeker policy) over N = num_policies policies, pairs_host
 * [G][2] i32 in HOST memory.  World w plays pairs[w mod G]; g = w / G is its group.  It is valid iff, checked in this
 * order: 1 <= N <= HS_LEAGUE_MAX_POLICIES; 1 <= G <= HS_LEAGUE_MAX_GROUP; every entry is in [0, N); it is REGULAR: every
 * policy holds the same number c = 2 G / N of sides per group, a pair (i, i) giving i two.  Regularity is exactly what
 * makes the routing a permutation with equal blocks of R / N slots, so hs_pack_policy_inputs_routed,
 * hs_sample_actions_routed and hs_compute_gae_grouped run on it as they are.
 * hs_league_set_schedule validates (HS_ERR_INVALID_ARG, nothing of the handle changed, hs_last_error says which rule),
 * builds the table the kernel reads (per pair the two policies and the sides each holds in the pairs before it, 16
 * bytes), uploads it into memory the handle owns and returns when it is there; pairs_host may be freed then.  group == 0
 * drops the schedule (pairs_host and num_policies are not looked at).  It is refused before hs_init and inside an open
 * step, and it must not overlap a league step in flight on this handle: the step reads the table, as it reads the step
 * table above.
 * hs_league_step_scheduled is hs_league_step with that schedule; the request is the same struct.  What differs:
 *   num_policies must equal the schedule's N, and the handle's number of worlds must be a multiple of G (not of N^2);
 *   with i, j = pairs[q], q = w mod G, and held[q][p] the sides p holds in pairs[0 .. q-1]: a hider row goes to policy
 *   i and a seeker row to j, and
 *     slot = p R / N + g c k + k held[q][p] + (the number of earlier rows of the world with the same policy);
 *   counts is [N][N][HS_LEAGUE_OUTCOMES], a game books into counts[i][j], and a pair that occurs more than once in the
 *   table books into the one cell; cells of pairs the table does not hold are never written.
 * Sides, malformed worlds, the latching, the outcomes, the Elo arithmetic (over all N policies, i == j moving nothing),
 * every other validation, the ordering and the stream rules are hs_league_step's, word for word; with the table
 * [(q / P, q % P) for q < P^2] every output has hs_league_step's bits.  Without a schedule set the call is refused with
 * HS_ERR_INVALID_ARG.  The set of slots a world owns does not change when its teams flip here either.  Setting a schedule
 * changes nothing for hs_league_step. */
#define HS_LEAGUE_MAX_GROUP 256   /* the pairs of a schedule table: HS_LEAGUE_MAX_POLICIES squared */
int32_t hs_league_set_schedule(hs_sim *sim, const int32_t *pairs_host, int32_t group, int32_t num_policies);
int32_t hs_league_step_scheduled(hs_sim *sim, const hs_league_request *req);
int32_t hs_league_step_scheduled_async(hs_sim *sim, void *hip_stream, const hs_league_request *req);

/* The routed pack: hs_pack_policy_inputs_normalized for a league or a population (one kernel, csrc/hs_k_pack_routed.h).
 * One launch packs every agent row into SLOT order, each row normalised with the table of the policy that owns the slot,
 * and collects the moments per policy.  With R = worlds * A rows and N = num_policies (R % N == 0), policy p owns slots
 * [p R / N, (p + 1) R / N), as hs_league_step lays them out; row_of_slot [R] i32 is what that call writes.
 *   Output row s (of actor and of critic, [R][HS_PACK_ROW], indexed by slot) has the BITS of row row_of_slot[s] of
 *   hs_pack_policy_inputs_normalized called with tables + (s / (R / N)) * HS_NORM_TABLE; with null tables, of
 *   hs_pack_policy_inputs.
 *   moments + p * moments_stride [HS_PACK_MOMENTS] f64, for every p: the sums over policy p's slots of m x, m x x and m of
 *   the raw f32 critic values, in f64, as hs_pack_policy_inputs states them.  No float atomics: the same inputs give the
 *   same bits on every call; with N == 1 and the identity routing they are the bits of hs_pack_policy_inputs.
 *   moments_stride is in doubles, >= HS_PACK_MOMENTS; nothing between the vectors is written.  A caller that keeps
 *   [N][T][HS_PACK_MOMENTS] hands base + t * HS_PACK_MOMENTS with stride T * HS_PACK_MOMENTS, so that each policy's T
 *   vectors are contiguous for hs_obs_norm_update.
 *   bad [1] i32 or null: zeroed by the call, then the number of slots whose row_of_slot is outside [0, R).  Such a slot's
 *   output rows are all-zero bits and it adds nothing to the moments; no export is read for it.
 * Validation as hs_pack_policy_inputs_normalized (HS_ERR_INVALID_ARG, nothing written), and in addition: null
 * row_of_slot; num_policies outside [1, HS_LEAGUE_MAX_POLICIES] or not a divisor of R; tables not 16-byte aligned;
 * moments given with moments_stride < HS_PACK_MOMENTS; row_of_slot or bad not 4-byte aligned; an output overlapping
 * row_of_slot, tables or another output.  The partial sums go through a workspace of the handle, so two calls with moments
 * on one handle must not overlap.  Ordering and streams as hs_pack_policy_inputs. */
typedef struct hs_pack_routed_request {
    void *actor;                  /* [R][HS_PACK_ROW] of actor_dtype, indexed by slot, or null */
    int32_t actor_dtype;          /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    void *critic;
    int32_t critic_dtype;
    const int32_t *row_of_slot;   /* [R] i32 */
    int32_t num_policies;         /* N in [1, HS_LEAGUE_MAX_POLICIES]; R % N == 0 */
    const float *tables;          /* [N][HS_NORM_TABLE] f32, 16-byte aligned, or null = no normalisation */
    double *moments;              /* policy p's [HS_PACK_MOMENTS] at moments + p * moments_stride, or null */
    int64_t moments_stride;       /* in doubles, >= HS_PACK_MOMENTS (read only with moments) */
    int32_t *bad;                 /* [1] i32 or null */
} hs_pack_routed_request;         /* 80 bytes */
int32_t hs_pack_policy_inputs_routed(hs_sim *sim, const hs_pack_routed_request *req);
int32_t hs_pack_policy_inputs_routed_async(hs_sim *sim, void *hip_stream, const hs_pack_routed_request *req);

/* The routed sampler: hs_sample_actions for a league or a population (one kernel, csrc/hs_k_sample_routed.h).  The logits
 * are in SLOT order (the P forwards write blocks of one buffer), the actions the next step reads go out in ROW order, and
 * what a learner stores stays in slot order.  With R = worlds * A rows and row_of_slot [R] i32 as hs_league_step writes it:
 *   For slot s with r = row_of_slot[s] in [0, R), action_rows[r] and action[s], log_prob[s], entropy[s], head_log_prob[s]
 *   have the BITS hs_sample_actions gives row r when it is handed a logits array whose row r is slot s's logits.
 *   The uniform is keyed by the global agent row world_offset * A + r, not by the slot: a draw does not depend on the
 *   routing.
 *   A slot whose row is outside [0, R) writes all-zero bits to its slot-order outputs, writes no row, and is counted in
 *   bad [1] i32 (or null), which the call zeroes first.  Rows named by no slot are left untouched.
 *   row_of_slot from hs_league_step is a permutation.  With duplicates the row holds one of its writers' quintuples;
 *   which one is unspecified.
 * mode is HS_SAMPLE_DRAW or HS_SAMPLE_GREEDY; HS_SAMPLE_EVALUATE is refused (an update scores stored actions with
 * hs_ppo_loss, which needs no routing).  flags must be 0.  action_rows null = the handle's action export.  action,
 * log_prob, entropy and head_log_prob may each be null.
 * Validation as hs_sample_actions (HS_ERR_INVALID_ARG, nothing written), and in addition: a null row_of_slot; a pointer
 * not 4-byte aligned (logits: their element size); an output overlapping logits, row_of_slot or another output, the
 * action export included when action_rows is null; every slot-order output null together with a non-null action_rows
 * (hs_sample_actions on gathered logits does that).  Ordering and streams as hs_sample_actions. */
typedef struct hs_sample_routed_request {
    const void *logits;           /* [R][logits_stride] of logits_dtype, indexed by slot */
    int32_t logits_dtype;         /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t logits_stride;        /* elements, >= sum of buckets */
    int32_t buckets[HS_SAMPLE_HEADS];
    int32_t mode;                 /* HS_SAMPLE_DRAW | HS_SAMPLE_GREEDY */
    uint32_t flags;               /* 0 */
    uint32_t seed[2];
    uint32_t counter;
    const int32_t *row_of_slot;   /* [R] i32 */
    int32_t *action_rows;         /* [R][5] indexed by ROW; null = the simulator's own action export */
    int32_t *action;              /* [R][5] indexed by slot, or null */
    float *log_prob, *entropy;    /* [R] indexed by slot, either may be null */
    float *head_log_prob;         /* [R][5] indexed by slot, or null */
    int32_t *bad;                 /* [1] i32 or null */
} hs_sample_routed_request;       /* 112 bytes */
int32_t hs_sample_actions_routed(hs_sim *sim, const hs_sample_routed_request *req);
int32_t hs_sample_actions_routed_async(hs_sim *sim, void *hip_stream, const hs_sample_routed_request *req);

/* Grouped advantages: hs_compute_gae with one moments vector per group of rows (csrc/hs_k_gae.h).  The rows are
 * `groups` = G groups of m = R / G consecutive rows: the slots of a population's policies.  advantage and returns are
 * exactly hs_compute_gae's (per-row chains).  moments is [G][HS_GAE_MOMENTS] f64: vector g has the BITS hs_compute_gae
 * writes on a handle of m rows that is given group g's columns as contiguous arrays (the grid is cut per group and each
 * group's partial sums are added in that call's order).  Validation as hs_compute_gae, the moments range being
 * G vectors, and in addition: groups outside [1, HS_LEAGUE_MAX_POLICIES] or not a divisor of R.  Workspace, ordering
 * and streams as hs_compute_gae. */
typedef struct hs_gae_grouped_request {
    hs_gae_request gae;           /* moments: [groups][HS_GAE_MOMENTS] f64 or null */
    int32_t groups;               /* G in [1, HS_LEAGUE_MAX_POLICIES]; R % G == 0 */
    int32_t reserved;             /* 0 */
} hs_gae_grouped_request;         /* 88 bytes */
int32_t hs_compute_gae_grouped(hs_sim *sim, const hs_gae_grouped_request *req);
int32_t hs_compute_gae_grouped_async(hs_sim *sim, void *hip_stream, const hs_gae_grouped_request *req);

/* The attention core of the entity self-attention encoder: what sits between the QKV GEMM and the output GEMM of the
 * reference's other network, EntitySelfAttentionNet(num_embed_channels=128, num_out_channels=256, num_heads=4)
 * (scripts/jax_policy.py), in one kernel each way (csrc/hs_k_attend.h).  madrona_learn is not part of the reference's
 * tree: the network around this call (gpu_hideseek.entity_attention) and the arithmetic below are the project's own and
 * are not pinned by it.
 * A row is S = HS_ATTEND_TOKENS = 17 tokens, the entities of a packed row in the order self, agents 0..4, boxes 0..8,
 * ramps 0..1, of E = embed_dim channels in H = HS_ATTEND_HEADS = 4 heads of D = E / 4 (E 64 or 128, D 16 or 32).
 * qkv [n][S][3][H][D] is the QKV GEMM's result viewed: q_i, k_i, v_i of token i and head h are the D elements from
 * ((i * 3 + {0, 1, 2}) * H + h) * D on.  key_mask [n][S] u8 (nonzero = the key counts) or null = every key counts; key 0
 * (self) counts whatever its byte says, so no softmax is empty.  out is [n][S][E], head h in the channels h D .. h D + D - 1.
 * The arithmetic is the contract.  Narrow inputs are widened to f32 exactly; everything is IEEE f32, unfused, in exactly
 * this order; expf is the device library's accurate function and is not pinned bit for bit.  For a row, head h, query i:
 *   dot(a, b) over a head's D channels: with P = D / 4, part g in 0..3 adds a_c * b_c for c = P g, ..., P g + P - 1 in
 *             ascending order (the first product is the start), then the parts add as a butterfly: every part t_g
 *             becomes t_g + t_{g xor 1}, then t_g + t_{g xor 2}, i.e. (t0 + t1) + (t2 + t3) up to commuted operands
 *   scale = 1.0f / sqrtf((float)D)                                  (correctly rounded; 0.25 at D = 16)
 *   s_j = dot(q_i, k_j) * scale                                     for the valid keys j
 *   m = the maximum of s_j over the valid keys, from s_0 on in ascending order (fmaxf)
 *   e_j = expf(s_j - m);   l = e_0, then l = l + e_j for the valid j >= 1 in ascending order
 *   p_j = e_j / l                                                   (division correctly rounded)
 *   out[i][h D + c] = ((+0 + p_j0 * v_j0[c]) + p_j1 * v_j1[c]) + ...   over the valid keys in ascending order
 * (rounded to out_dtype to nearest even).  A masked key is left out BY A SELECT, not by a multiplication with 0: its k and
 * v may hold NaN or Inf and every output keeps its bits.  A masked QUERY is computed like any other (the caller's pool
 * drops it).  No atomics, no workspace: a row's bits do not depend on n, on its position or on its neighbours, and the
 * same inputs give the same bits on every call.
 * hs_entity_attend_backward recomputes p from q, k and the mask exactly as above (the forward saves nothing) and takes
 * grad_out [n][S][E] of grad_dtype; grad_qkv has the shape of qkv and grad_dtype:
 *   dp_ij = dot(dout_i, v_j)                                        for the valid keys j (dout_i: head h's D channels)
 *   t_i = ((+0 + p_ij0 * dp_ij0) + p_ij1 * dp_ij1) + ...            over the valid keys in ascending order
 *   ds_ij = p_ij * (dp_ij - t_i)
 *   dq_i[c] = (((+0 + ds_ij0 * k_j0[c]) + ds_ij1 * k_j1[c]) + ...) * scale     over the valid keys in ascending order
 *   dv_j[c] = ((+0 + p_0j * dout_0[c]) + p_1j * dout_1[c]) + ... + p_16j * dout_16[c]       every query, ascending
 *   dk_j[c] = (((+0 + ds_0j * q_0[c]) + ds_1j * q_1[c]) + ... + ds_16j * q_16[c]) * scale
 *   dk_j and dv_j of a masked key are exactly +0 (a select).
 * There are no parameters, hence no sum over rows.  An all-zero grad_out gives grad_qkv all +0.  q, the valid keys' k and
 * v, and grad_out must be finite: nothing checks that on the device.
 * A lane reads and writes pieces of 4 adjacent elements (up to 16 bytes), so qkv, out, grad_out and grad_qkv must be
 * 16-byte aligned, as for hs_dense_norm_act.  Elements are indexed in 64 bits, so n * S * 3 * E may pass 2^31; n itself stays
 * below HS_ATTEND_MAX_ROWS.
 * Everything is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a
 * null request, null qkv or out (backward: null grad_out or grad_qkv); an unknown dtype; embed_dim not 64 or 128; n < 1
 * or n >= 2^24; a pointer not 16-byte aligned (key_mask: any); an output range that overlaps an input range; a call before
 * hs_init or inside an open step.  The calls read no export and write no simulator state, and any number of them may
 * overlap on one handle.  The blocking forms are ordered after the device's legacy default stream; the _async forms
 * enqueue on the caller's hipStream_t without synchronising. */
enum { HS_ATTEND_TOKENS = 17, HS_ATTEND_HEADS = 4, HS_ATTEND_ROWS_PER_ROUND = 4, HS_ATTEND_MAX_GRID = 2048, HS_ATTEND_MAX_ROWS = 1 << 24 };
typedef struct hs_entity_attend_request {
    const void    *qkv;           /* [n][HS_ATTEND_TOKENS][3][HS_ATTEND_HEADS][embed_dim / 4] of qkv_dtype, contiguous, 16-byte aligned */
    const uint8_t *key_mask;      /* [n][HS_ATTEND_TOKENS] u8, nonzero = valid, or null = all valid */
    int32_t n;                    /* rows, 1 <= n < HS_ATTEND_MAX_ROWS */
    int32_t embed_dim;            /* E: 64 or 128 (the reference's) */
    int32_t qkv_dtype;            /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t out_dtype;            /* of out */
    void    *out;                 /* [n][HS_ATTEND_TOKENS][embed_dim] of out_dtype, 16-byte aligned */
} hs_entity_attend_request;       /* 40 bytes */
typedef struct hs_entity_attend_backward_request {
    const void    *qkv;           /* as in the forward call */
    const uint8_t *key_mask;
    const void    *grad_out;      /* [n][HS_ATTEND_TOKENS][embed_dim] of grad_dtype, 16-byte aligned */
    int32_t n;
    int32_t embed_dim;
    int32_t qkv_dtype;
    int32_t grad_dtype;           /* of grad_out and grad_qkv */
    void    *grad_qkv;            /* the shape of qkv, of grad_dtype, 16-byte aligned */
} hs_entity_attend_backward_request;  /* 48 bytes */
int32_t hs_entity_attend(hs_sim *sim, const hs_entity_attend_request *req);
int32_t hs_entity_attend_async(hs_sim *sim, void *hip_stream, const hs_entity_attend_request *req);
int32_t hs_entity_attend_backward(hs_sim *sim, const hs_entity_attend_backward_request *req);
int32_t hs_entity_attend_backward_async(hs_sim *sim, void *hip_stream, const hs_entity_attend_backward_request *req);

/* The SimHash encoder: the reference's HashNet (scripts/jax_policy.py:170-218, the network make_policy selects with
 * use_hash=True) over rows of hs_pack_policy_inputs.  HashNet concatenates self, agents, boxes and ramps, which is the
 * row's column order, projects the HS_PACK_ROW columns onto HS_HASH_BITS directions, takes the sign bits as a bin number
 * 0 .. HS_HASH_BINS - 1, looks the bin up in a table of HS_HASH_FEATURES channels and LayerNorms the looked-up row.  The
 * reference's hash_power = 8 and feature_dim = 32 are fixed.  One kernel (csrc/hs_k_hash.h) reads a row once and writes
 * its bin and its 32 channels; n is free, as for hs_ppo_loss.
 * params is one array of HS_HASH_PARAMS f32: proj [8][296] (direction major), table [256][32], then the LayerNorm's
 * scale (gamma) [32] and shift (beta) [32].
 * The arithmetic is the contract.  Narrow rows are widened to f32 exactly; everything is IEEE f32, unfused except where
 * fmaf is written, in exactly this order.  For a row x_0 .. x_295 and bit i < 8, with 64 lanes l:
 *   p_l = +0;   p_l = fmaf(x_k, proj[i][k], p_l)   for k = l, l + 64, l + 128, l + 192 and, where l < 40, l + 256
 *   y_i = the butterfly over the 64 lanes: for m = 1, 2, 4, 8, 16, 32 every lane replaces s_l by s_l + s_{l xor m}
 *         (every lane ends with the same bits; it is hs_entity_encode's sum_c with L = 64)
 *   bit_i = y_i > 0    (a NaN or an exact zero gives 0, so an all-zero row lands in bin 0);   bin = sum_i bit_i << i
 * The order depends on nothing but the row: not on n, on the row's index, on the grid or on rows_dtype.
 *   LayerNorm of table row b (hs_entity_encode's expression with E = 32 and its sum_c with L = 32):
 *   mu = sum_c(t_c) / 32.0f;   d_c = t_c - mu;   var = sum_c(d_c * d_c) / 32.0f;   rstd = 1.0f / sqrtf(var + eps)
 *   that_c = d_c * rstd;   T[b][c] = fmaf(that_c, gamma_c, beta_c)
 *   features[row][c] = T[bin][c], rounded once to features_dtype, to nearest even
 * A workgroup normalises the 256 table rows once, into LDS, and every row it takes is one gather: T depends on params and
 * eps alone, so every workgroup holds the same bits.  eps = 1e-6 is flax's default; the reference's LayerNorm comes from
 * madrona_learn, which is not part of its tree, so the constant is not pinned by it.
 * hs_hash_encode_backward takes the forward's bin, the upstream grad_features [n][32] and params, and writes grad_params
 * [HS_HASH_PARAMS] f32 in the layout of params.  The hash is a step function and the reference puts stop_gradient on it:
 * there is no gradient with respect to proj or the rows, and the whole proj range of grad_params is written +0.  The
 * LayerNorm's backward is linear in the incoming gradient, so the gradients are summed per bin first:
 *   G[b][c] = the sum of grad_features[r][c] (widened exactly) over the rows r with bin_r = b, in this order, which depends
 *     on n alone: with R = HS_HASH_ROWS_PER_ROUND rows per round and W = min(ceil(n / R), HS_HASH_MAX_GRID_BWD)
 *     workgroups, workgroup w takes rounds w, w + W, ...; wave v of it the rows round * R + 2 v + s (s = 0, 1) and adds
 *     them onto a slice [256][32] of its own that starts as +0, in round order and s = 0 before s = 1; the waves' slices
 *     are added as ((v0 + v1) + v2) + v3; the workgroups' sums go to a workspace of the handle, where HS_HASH_SUM_SEGS
 *     segments of ceil(W / segs) consecutive workgroups are each added in ascending order onto +0 and the segments then
 *     in ascending order (the kernel that does so is hs_entity_encode_backward's)
 *   h_c = gamma_c * G[b][c];   mh = sum_c(h_c) / 32.0f;   mhz = sum_c(h_c * that_c) / 32.0f
 *   d table[b][c] = rstd * ((h_c - mh) - that_c * mhz), and +0 for a bin whose G[b] is 0 in every channel: a bin without
 *     rows gets +0 by bit pattern
 *   d gamma_c: HS_HASH_SUM_SEGS segments of 32 consecutive bins each start from +0 and take s = fmaf(G[b][c], that_c, s)
 *     in ascending b; the segments are added in ascending order.  d beta_c the same with s = s + G[b][c].
 * No atomics: the same inputs give the same bits on every call, and a row's bin and features do not depend on its
 * position or on n.  grad_features all zero gives grad_params all +0.
 * Rows may hold anything (a NaN in a column only clears bits); params and grad_features must be finite: nothing checks
 * that on the device.  Two backward calls on one handle must not overlap (the workspace); forward calls may.  Everything
 * is validated before anything is launched (HS_ERR_INVALID_ARG, nothing written, hs_last_error says which): a null
 * request, null rows, params or features (backward: a null bin, grad_features, params or grad_params); an unknown dtype;
 * n < 1 or n * 296 >= 2^31; eps not finite or <= 0; rows not 16-byte aligned, features or grad_features not aligned to
 * their element size, params or grad_params not 4-byte aligned; an output range that overlaps an input range or another
 * output; a call before hs_init or inside an open step.  The calls read no export and write no simulator state.  The
 * blocking forms are ordered after the device's legacy default stream; the _async forms enqueue on the caller's
 * hipStream_t without synchronising. */
enum { HS_HASH_BITS = 8, HS_HASH_BINS = 256, HS_HASH_FEATURES = 32, HS_HASH_PARAMS = 8 * 296 + 256 * 32 + 32 + 32,
       HS_HASH_ROWS_PER_ROUND = 8, HS_HASH_MAX_GRID_BWD = 256, HS_HASH_SUM_SEGS = 8 };
typedef struct hs_hash_encode_request {
    const void    *rows;          /* [n][HS_PACK_ROW] of rows_dtype, contiguous, 16-byte aligned */
    const float   *params;        /* [HS_HASH_PARAMS] f32 */
    int32_t n;                    /* rows, n >= 1 */
    int32_t rows_dtype;           /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    int32_t features_dtype;       /* of features */
    float eps;                    /* finite, > 0; 1e-6 */
    void    *features;            /* [n][HS_HASH_FEATURES] of features_dtype */
    uint8_t *bin;                 /* [n], or null */
} hs_hash_encode_request;         /* 48 bytes */
typedef struct hs_hash_encode_backward_request {
    const uint8_t *bin;           /* [n], what the forward call wrote */
    const void    *grad_features; /* [n][HS_HASH_FEATURES] of grad_dtype */
    const float   *params;        /* as in the forward call */
    int32_t n;
    int32_t grad_dtype;           /* HS_DTYPE_F32 | HS_DTYPE_BF16 | HS_DTYPE_F16 */
    float eps;
    int32_t reserved;             /* ignored */
    float   *grad_params;         /* [HS_HASH_PARAMS] f32 */
} hs_hash_encode_backward_request;  /* 48 bytes */
int32_t hs_hash_encode(hs_sim *sim, const hs_hash_encode_request *req);
int32_t hs_hash_encode_async(hs_sim *sim, void *hip_stream, const hs_hash_encode_request *req);
int32_t hs_hash_encode_backward(hs_sim *sim, const hs_hash_encode_backward_request *req);
int32_t hs_hash_encode_backward_async(hs_sim *sim, void *hip_stream, const hs_hash_encode_backward_request *req);

/* The XLA-callable entry points behind `sim.jax()` (src/bindings.cpp:97-118): enqueue on the caller's
 * hipStream_t, device buffers in the reference's order, no synchronisation except hs_jax_init.
 *   obs block (JAXIOObservations, mgr.cpp:168-201): prep_counter, self_data, self_type, self_mask, lidar,
 *   agent_data, box_data, ramp_data, vis_agents_mask, vis_boxes_mask, vis_ramps_mask.
 * hs_jax_init  (gpuStreamInit mgr.cpp:362-376):  buffers = obs block (out).
 * hs_jax_step  (gpuStreamStep mgr.cpp:379-398):  buffers = actions, resets, policy_assignments (in), obs block,
 *                                                rewards, dones, episode_results (out).
 * hs_jax_save_checkpoints (mgr.cpp:400-416):     buffers = ckpt_ctrl (in), ckpts (out).
 * hs_jax_load_checkpoints (mgr.cpp:418-436):     buffers = ckpt_ctrl, ckpts (in), obs block (out). */
int32_t hs_jax_init(hs_sim *sim, void *hip_stream, void **buffers);
int32_t hs_jax_step(hs_sim *sim, void *hip_stream, void **buffers);
int32_t hs_jax_save_checkpoints(hs_sim *sim, void *hip_stream, void **buffers);
int32_t hs_jax_load_checkpoints(hs_sim *sim, void *hip_stream, void **buffers);

/* The same four functions as XLA GPU custom-call targets — what madrona::py::JAXInterface::buildEntry
 * (src/bindings.cpp:97-118) registers with XLA: `void target(stream, buffers, opaque, opaque_len)`, the original
 * status-less custom-call ABI; XLA passes its hipStream_t, the operand and result device buffers in call order (the
 * orders above) and the descriptor the Python side attached — the 8 bytes of the hs_sim* handle.  A failure cannot be
 * returned through this ABI: it is kept, hs_xla_last_status(clear) reports it, and the next blocking call on the
 * handle returns HS_ERR_HIP.  `sim.jax()` wraps the four addresses in PyCapsules named "xla._CUSTOM_CALL_TARGET". */
void hs_xla_init(void *hip_stream, void **buffers, const char *opaque, size_t opaque_len);
void hs_xla_step(void *hip_stream, void **buffers, const char *opaque, size_t opaque_len);
void hs_xla_save_checkpoints(void *hip_stream, void **buffers, const char *opaque, size_t opaque_len);
void hs_xla_load_checkpoints(void *hip_stream, void **buffers, const char *opaque, size_t opaque_len);
int32_t hs_xla_last_status(int32_t clear);

/* Manager::trainInterface (src/mgr.cpp:1338-1375): the names and roles under which `sim.jax()` hands the exported
 * tensors to the learner, in the reference's order (which is also the buffer order of hs_jax_step).  `export_id` is
 * an HS_EXPORT_* value, or -1 for the empty simCtrl tensor (mgr.cpp:1333-1336).  Returns the number of entries and
 * points *entries at a static table. */
enum {
    HS_ROLE_ACTION = 0,        /* TrainInterface inputs.actions */
    HS_ROLE_RESET = 1,         /* inputs.resets */
    HS_ROLE_SIM_CTRL = 2,      /* inputs.simCtrl (empty) */
    HS_ROLE_PBT_INPUT = 3,     /* inputs.pbt */
    HS_ROLE_OBSERVATION = 4,   /* outputs.observations */
    HS_ROLE_REWARD = 5,        /* outputs.rewards */
    HS_ROLE_DONE = 6,          /* outputs.dones */
    HS_ROLE_PBT_OUTPUT = 7,    /* outputs.pbt */
    HS_ROLE_CHECKPOINT = 8     /* TrainCheckpointingInterface.checkpointData */
};
typedef struct hs_iface_entry {
    const char *name;
    int32_t role;
    int32_t export_id;
} hs_iface_entry;
int32_t hs_train_interface(const hs_iface_entry **entries);

/* Device-side conditions the reference has no channel for (it asserts or aborts).
 *   spilled_dd_pairs / spilled_static_pairs: broadphase candidate pairs of a world beyond what the physics kernel keeps
 *     in LDS per substep (16 body-body, 24 body-static).  They are NOT lost: they go through a global spill list sized
 *     for the worst case (17 bodies: 136 pairs; 17 x 38 statics — the reference sizes for every entity too,
 *     src/sim.cpp:1356-1361) and are tested and solved in the same order as every other pair, on a slower path; results
 *     are identical to an unbounded solver.  Sticky totals since hs_create; a performance signal, not an error.
 *   dropped_dd_pairs / dropped_static_pairs: candidate pairs discarded.  Always 0 (nothing can overflow the spill
 *     lists); kept so that callers can assert it (bench.py, tools/train_config_bench.py do).
 *   graphs_in_use: always 0 (HIP-graph replay was removed); the field keeps the layout.
 *   split_steps: blocking steps (hs_step) that ran as two chains, late and early octets, since hs_create; late_octets:
 *     the octets of their late groups, summed over those steps (hs_set_late_threshold). */
typedef struct hs_device_status {
    int64_t dropped_dd_pairs;
    int64_t dropped_static_pairs;
    int32_t graphs_in_use;
    int32_t reserved;
    int64_t spilled_dd_pairs;
    int64_t spilled_static_pairs;
    int64_t split_steps;
    int64_t late_octets;
} hs_device_status;
int32_t hs_get_device_status(hs_sim *sim, hs_device_status *out);

/* The one tunable of the split schedule of the blocking hs_step: the octets (8 worlds, one physics
 * wave) whose mean time over the last two steps exceeded `factor` x the mean over all octets form the late group of the
 * next step, the others the early group; the two groups run as independent k_physics -> k_observe chains on two
 * streams.  A parameter of that one schedule, not a switch: 0 makes every octet late, a huge value (values above 1e6
 * are taken as 1e6) nobody, and one launch of each pair then finds no octet to serve.  Results do not depend on it.
 * The default is fixed by measurement.  Takes effect from the groups the next step forms, i.e. one step later. */
int32_t hs_set_late_threshold(hs_sim *sim, float factor);

/* maxAgentsPerWorld (src/mgr.cpp:684). */
int32_t hs_agents_per_world(const hs_sim *sim);

/* Internal-state dumps (not in the reference; used by the parity tests and by INTEGRATION.md's
 * shard-equivalence check).  Host output buffers:
 *   bodies [num_worlds][17][13] f32 = pos3 rot4(wxyz) lin3 ang3, meta [num_worlds][17][3] i32 =
 *   objType, response, owner;  walls [num_worlds][36][4] f32 = cx cy hx hy,
 *   info [num_worlds][8] i32 = numWalls numPlanes numActiveBoxes numActiveRamps numHiders numSeekers
 *   curEpisodeStep seekersFirst. */
int32_t hs_debug_dump_bodies(hs_sim *sim, float *bodies, int32_t *meta);
int32_t hs_debug_dump_walls(hs_sim *sim, float *walls, int32_t *info);

/* Milliseconds of device time of the last `hs_step`, measured with HIP events on the launch stream when
 * profiling is enabled: [0] k_physics (movement / actions, 4 XPBD substeps, rewards), [1] k_reset,
 * [2] k_observe. */
int32_t hs_set_profiling(hs_sim *sim, int32_t enabled);
int32_t hs_last_step_kernel_ms(hs_sim *sim, float out_ms[3]);

/* Development aid: per-phase wall-clock ticks (100 MHz) accumulated by every workgroup of the physics kernel,
 * [groups][10] = pre, integrate, detect, sat, dd_pos, body_pos, dd_vel, body_vel, post, -; all zero unless the
 * library was built with -DHS_PHASE_TIMING.  Returns the number of groups written (<= max_groups). */
int32_t hs_debug_phase_ticks(hs_sim *sim, int64_t *out, int32_t max_groups);
/* The same for k_observe: ticks per section, summed over all waves: stage (incl. the schedule's wait), per-agent table,
 * ray setup, walls, planes, hull cull, exact hull tests, ray results, observation rows. */
int32_t hs_debug_observe_ticks(hs_sim *sim, int64_t out[16]);

/* The DEVICE's hull tables for one SimObject (src/sim.hpp:78-88; 3 = wall, unit size), evaluated by a one-lane kernel through
 * the very functions the convex tests use (csrc/hs_collide.h: packed topology, closed-form vertices) at the identity
 * pose: verts [8][3], faces [6][4] (-1 padded), counts {nv, nf, ne, ned}, normals [6][3], edges [12][3] = v0 v1 dir,
 * local [8][3] = hull_local_vertex (the contact points of plane manifolds).  tests/test_gpu_hulls.py pins them to
 * tests/golden/hulls.npz, i.e. to data/{cube,wall,agent,ramp,elongated}_collision.obj of the reference. */
int32_t hs_debug_dump_hull(int32_t obj, float *verts, int32_t *faces, int32_t *counts, float *normals, int32_t *edges,
                           float *local);

/* The DEVICE's object table for one SimObject: out[6] = inverse mass, static / dynamic friction coefficient, inverse inertia x y z
 * (object frame) as the kernels use them (csrc/hs_core.h, the scalar core the CPU oracle reads too).  tests/test_gpu_hulls.py pins the first three and the zeroed
 * inertia axes of the agents to tests/golden/object_table.json (src/mgr.cpp:441-588). */
int32_t hs_debug_object_params(int32_t obj, float *out);

/* The DEVICE's reading of the scalar core's probe table (csrc/hs_core_probe.h, which lists the ops and their operands): `n`
 * cases of 16 words in host memory `in`, 16 words each to host memory `out`, one case per lane.  Integer operands and results
 * travel as bit patterns.  HS_ERR_INVALID_ARG, and nothing written, for a null pointer, n <= 0, n > 1 << 20 or an unknown op.
 * tests/test_gpu_core_probe.py compares it bit for bit with the CPU oracle's reading of the same text (hsref_core_eval). */
int32_t hs_debug_core_eval(int32_t op, int32_t n, const float *in, float *out);

/* Profiling aid: one dword-per-lane coalesced copy of `bytes` bytes (read + write), used to calibrate the
 * rocprofv3 FETCH_SIZE / WRITE_SIZE counters for the simulator's access pattern. */
int32_t hs_debug_calibrate(int64_t bytes);

/* No-op `DLManagedTensor::deleter` for the non-owning DLPack views built by language bindings. */
void hs_dlpack_noop_deleter(void *managed_tensor);

const char *hs_last_error(void);
const char *hs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HIDESEEK_H */
