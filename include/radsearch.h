/*
 * radsearch.h -- C ABI of the MI355X-native radiation-search PPO hot path (librs_hip.so).
 *
 * The reference (bentotten/radiation_ppo) has no plugin/FFI interface: its boundary is two Python
 * call surfaces.  This ABI sits directly behind them; every entry point names the reference
 * interface it replaces (paths relative to the reference root):
 *
 *   rs_step      <- RadSearch.step            gym_rad_search/gym_rad_search/envs/rad_search_env.py:443-728
 *   rs_reset     <- RadSearch.reset           rad_search_env.py:730-797 (+ create_obs :948-1011,
 *                                             sample_source_loc_pos :1013-1131)
 *   rs_set_epoch_end <- `env.epoch_end = True` algos/multiagent/train.py:482-484
 *   rs_gae       <- PPOBuffer.GAE_advantage_and_rewardsToGO   algos/multiagent/ppo.py:391-423
 *                   (discount_cumsum ppo.py:62-85), one call for the whole [T, N*A] buffer
 *
 * Conventions
 *   - plain C: pointers and sizes only, no torch types, no exceptions; return 0 = RS_OK.
 *   - every pointer marked "device" is HBM owned by the CALLER (PyTorch tensors in the Python host);
 *     the library borrows it for the duration of the call's stream-ordered work.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); nothing synchronises.
 *   - no allocation after rs_create; one handle per device; a handle is not thread-safe.
 *   - environments are independent: a multi-GPU job gives each rank its own handle with
 *     env_id_base = first global env id of the rank (results do not depend on the sharding).
 */
#ifndef RADSEARCH_H
#define RADSEARCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ABI_VERSION 4
#define RS_OBS_DIM 11      /* [measurement, x/scale, y/scale, 8 range sensors]  rad_search_env.py:589-593 */
#define RS_NUM_ACTIONS 9   /* 0..7 directions, 8 idle                           rad_search_env.py:55-68  */
#define RS_MAX_AGENTS 8
#define RS_MAX_OBS 7       /* obstruction_count in {-1,0..7}                    rad_search_env.py:315,327 */

typedef void* rs_stream_t; /* hipStream_t */
typedef struct rs_handle rs_handle;

enum {
    RS_OK = 0,
    RS_ERR_INVALID_ARG = 1,
    RS_ERR_HIP = 2,
    RS_ERR_WORKSPACE = 3,
    RS_ERR_UNSUPPORTED = 4
};

/* per-env error bits accumulated on the device (conditions on which the reference raises) */
enum {
    RS_ENVERR_ZERO_DIST = 1,   /* detector on the source: intensity / 0 (rad_search_env.py:501)            */
    RS_ENVERR_IDLE_STALL = 2,  /* idle action stalled without collision (ValueError, :544-547, :562-565)  */
    RS_ENVERR_CORRECT_CAP = 4, /* correct_coords loop (:1278) hit the iteration cap                       */
    RS_ENVERR_BAD_ACTION = 8,  /* action outside 0..8 / -1 (assert, :616-627)                             */
    RS_ENVERR_NO_PATH = 16     /* no obstacle-free path detector -> source (cannot happen in a valid world) */
};

typedef struct rs_config {
    int32_t num_envs;                /* N: envs owned by this handle                                   */
    int32_t num_agents;              /* A: 1..RS_MAX_AGENTS (number_agents, rad_search_env.py:354)     */
    int32_t obstruction_count;       /* -1 => U{1..5} per epoch, 0 none, 1..7 (rad_search_env.py:327)  */
    int32_t enforce_grid_boundaries; /* rad_search_env.py:328                                          */
    int32_t bbox[4];                 /* x0,y0,x1,y1 in cm (default 0,0,2700,2700; :320-324)            */
    int32_t observation_area[2];     /* (200,500) (:325)                                               */
    int32_t falloff;                 /* 0 = as written in the reference, I/r (:501); 1 = I/r^2         */
    int32_t geom_group_size;         /* envs sharing one obstacle layout; 1 = reference-faithful       */
    uint32_t seed;                   /* Philox key word 0                                              */
    uint32_t env_id_base;            /* global id of local env 0 (Philox key word 1 = base + n)        */
    int32_t coord_noise;             /* coord_noise (rad_search_env.py:365, :569-580): N(0, 5 cm) on the two coordinates of the
                                        OBSERVATION (not of the state), a fresh pair per agent-step (Philox stream 96 + agent) */
    int32_t debug_spawn;             /* DEBUG (:387-389, :782-785, :1043-1090): source (500, 500), detector (1000, 1000), no
                                        minimum-distance / line-of-sight resampling, intensity 1e6, background 0             */
} rs_config;

/* optional per-agent info outputs of rs_step / rs_reset (any pointer may be NULL); all device, [N,A] */
typedef struct rs_info {
    uint8_t* out_of_bounds;       /* info["out_of_bounds"]        rad_search_env.py:607-612 */
    int32_t* out_of_bounds_count; /* info["out_of_bounds_count"]                            */
    uint8_t* blocked;             /* info["blocked"] (sticky per episode)                   */
    uint8_t* collision;           /* Agent.collision (:268)                                 */
} rs_info;

/* ---- lifecycle ----------------------------------------------------------------------------- */
const char* rs_strerror(int code);
int rs_abi_version(void);

/* bytes of device workspace a handle needs for `cfg` (0 on invalid cfg) */
size_t rs_state_bytes(const rs_config* cfg);

/* workspace: device memory of >= rs_state_bytes(cfg) bytes, 256-byte aligned, owned by the caller
 * and kept alive until rs_destroy.  Zero-fills it on `stream`; every env starts with epoch_end set
 * (rad_search_env.py:421) and must be rs_reset before the first rs_step. */
int rs_create(const rs_config* cfg, void* workspace, size_t workspace_bytes, rs_stream_t stream, rs_handle** out);
void rs_destroy(rs_handle* h);

/* introspection for tests/adapters: device pointer + shape of one SoA state field.
 * names: "src_x","src_y","intensity","bkg","iter_count","episode","tstep","err","done","epoch_end"
 * ([N]); "num_obs" ([G]); "rect" ([28,G] int32: (obstacle*4 + {x0,y0,x1,y1}) major); "dsrc" ([28,N] f64);
 * "x","y","oob_count" ([A,N] int32); "sp","prev" ([A,N] f64); "aflags" ([A,N] u8: bit0 blocked,
 * bit1 intersect, bit2 out_of_bounds, bit3 collision).  elem: 1,4,8 bytes. */
int rs_state_field(rs_handle* h, const char* name, void** dev_ptr, int32_t* elem_bytes, int32_t* rows, int32_t* cols);

/* ---- environment ----------------------------------------------------------------------------- */
/* `env.epoch_end = True` for every env: the next rs_reset of an env resamples its obstacle layout. */
int rs_set_epoch_end(rs_handle* h, rs_stream_t stream);

/* Reset the envs whose mask byte is non-zero (mask == NULL: all).  For those envs writes the initial
 * observation (the reference's `step(None)`), reward, team reward, done and info rows; other rows are
 * left untouched.  obs [N,A,11] f32, reward [N,A] f32, team [N] f32, done [N,A] u8 (any may be NULL). */
int rs_reset(rs_handle* h, const uint8_t* mask, float* obs, float* reward, float* team, uint8_t* done,
             const rs_info* info, rs_stream_t stream);

/* RadSearch.refresh_environment (rad_search_env.py:799-874): start the masked envs' episodes from SAVED parameters
 * instead of sampling them (the evaluation harness replays its test-environment sets this way, evaluate.py:346).
 * src_xy, det_xy [N][2] int32 (cm), intensity, bkg [N] int32; num_obs [N] + rects [N][7][4] int32 (x0,y0,x1,y1) replace
 * the obstacle layout, or both NULL to keep the env's current one (the reference's num_obs = 0 default).  Outputs as
 * rs_reset (the observation of the idle step the reference takes); afterwards iter_count = 1 as in the reference. */
int rs_refresh(rs_handle* h, const uint8_t* mask, const int32_t* src_xy, const int32_t* det_xy, const int32_t* intensity,
               const int32_t* bkg, const int32_t* num_obs, const int32_t* rects, float* obs, float* reward, float* team,
               uint8_t* done, const rs_info* info, rs_stream_t stream);

/* One lock-step of all N envs.  actions [N,A] int8: 0..8 (-1 == idle 8) = the dict form of RadSearch.step with the
 * collision rule (rad_search_env.py:645-659); 9 = the reference's step(None) for that agent (no move, stale distances,
 * :528-567); 16 + a (a in 0..8) = the single-int form `step(a)` (:676-690): action a for the agent, and when ANY agent of
 * an env carries this form no collision rule is applied in that env (the reference calls agent_step without
 * proposed_coordinates there).  Outputs as rs_reset.
 * done[n,a] is the env-wide latch as seen when agent a returned (rad_search_env.py:509,613). */
int rs_step(rs_handle* h, const int8_t* actions, float* obs, float* reward, float* team, uint8_t* done,
            const rs_info* info, rs_stream_t stream);

/* Uniforms for action sampling, u[n,a] in [0,1) with 24 random bits, from the env's own Philox stream:
 * key (seed, global env id), counter (0, step index of the NEXT rs_step, episode, 32 + a).  The host
 * (and the fused collector) sample a = #{j : cdf_j <= u}, so a trajectory is a pure function of
 * (seed, env id, policy).  Replaces Categorical(probs).sample() (FF_core.py:101-104). */
int rs_action_uniforms(rs_handle* h, float* u, rs_stream_t stream);

/* Test probe of the measurement draw: draw d = Poisson(lam[d]) with key (seed, env_id[d]) and counter (candidate, t[d], episode[d],
 * 1), as agent 0's measurement in rs_step.  serial[d]: the serial sampler every kernel but the fused rollout uses; group3[d] /
 * group4[d]: the fused rollout's grouped sampler with 3 / 4 candidates evaluated side by side (the rollout uses 3); candidates[d]:
 * how many candidates the serial rejection loop consumed (0 for lam < 10, which has no such loop).  The three values must agree.
 * Rates outside [0, 1e12] are drawn as 0.  All arrays [count], on the device. */
int rs_poisson_probe(const double* lam, const uint32_t* t, const uint32_t* episode, const uint32_t* env_id, int64_t count, uint32_t seed,
                     int64_t* serial, int64_t* group3, int64_t* group4, int32_t* candidates, rs_stream_t stream);

/* host copy of the OR of all per-env error bits (synchronises `stream`; debugging/adapters only) */
int rs_error_flags(rs_handle* h, rs_stream_t stream, uint32_t* flags_out);

/* ---- PPO buffer math ------------------------------------------------------------------------ */
/* GAE(lambda) advantages and rewards-to-go for a whole rollout buffer, time-major [T, M] (M = N*A
 * columns, one trajectory stream per column).  cut[t,m] != 0: the trajectory of column m ends after
 * step t and last_val[t,m] is its bootstrap value (V(s_T) on timeout / epoch cut, 0 on terminal,
 * train.py:462-487).  Computed in float64 per column exactly as scipy.lfilter does, stored float32. */
int rs_gae(const float* rew, const float* val, const uint8_t* cut, const float* last_val, float* adv, float* ret,
           int32_t T, int32_t M, double gamma, double lam, rs_stream_t stream);

/* What one rank's PPO update takes from the finished buffer of a single-agent collector, time-major [T, N], in three launches:
 *   w[t,n]     = (1 / (episodes of column n * length of the episode step t lies in)) * float32(1 / n_total), float32 operations in
 *                that order (RolloutBuffer.episode_weights() / n_total, where the tensor library divides by a Python number through
 *                its reciprocal; cut[t,n] != 0 ends an episode, the last step always ends one);
 *   mean_std   = { float32(sum(adv) / (T*N)), float32(sqrt(sum(float32((adv - mean)^2)) / (T*N))) }, both sums float64
 *                (PPOBuffer.get's normalisation, ppo.py:445-446, population std, no epsilon);
 *   adv_n[t,n] = (adv[t,n] - mean) / std.  adv itself is left as it is.
 * The sums run in a fixed order without atomics: the same buffer gives the same bits.  workspace: rs_ppo_prepare_workspace_bytes(N)
 * bytes, 8-byte aligned, device. */
size_t rs_ppo_prepare_workspace_bytes(int32_t N);
int rs_ppo_prepare(const uint8_t* cut, const float* adv, float* w, float* adv_n, float* mean_std, void* workspace, int32_t T, int32_t N,
                   int32_t n_total, rs_stream_t stream);

/* ---- policy (FF_core.ActorCritic, NeuralNetworkCores/FF_core.py:42-129) ---------------------- */
/* One 2x64 tanh MLP in torch layout: w1 [64,11], b1 [64], w2 [64,64], b2 [64], w3 [out,64], b3 [out]
 * (row-major [out][in] float32, i.e. nn.Linear.weight / .bias of actor.0/.2/.4 or critic.0/.2/.4). */
typedef struct rs_mlp_params {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
} rs_mlp_params;

/* actor logits [M,8] (pre-softmax: actor.4 output) and critic value [M] for M observations x [M,11] on the
 * matrix cores (v_mfma_f32_32x32x2_f32, exact f32).  Replaces ActorCritic.actor / .critic forward
 * (FF_core.py:95-129).  Any of logits / value may be NULL. */
int rs_policy_forward(const rs_mlp_params* actor, const rs_mlp_params* critic, const float* x, int32_t M,
                      float* logits, float* value, rs_stream_t stream);

/* One round of ac.step for every agent of a feed-forward team (train.py:345-357, :476-480; FF_core.py:95-129): agent a's own actor
 * and critic on its own rows x[n][a][:].  One launch, grid = (64-sample groups, agent); the forward pass is rs_policy_forward's.
 *   actors, critics [A]   host arrays of rs_mlp_params (device pointers inside), A = num_agents in 1..RS_MAX_AGENTS
 *   x [N][A][11]
 *   u [N][A] != NULL: the step round.  act [A][N] int64 = #{j < 7 : cdf_j <= u}, logp_val_boot [A][3][N]: slot 0 = log-softmax at the
 *        action, slot 1 = value; act8 [N][A] (rs_step's action rows) receives the action once more.  mask is ignored.
 *   u == NULL: the bootstrap round.  slot 2 of logp_val_boot = value, for the envs with mask[n] != 0 (all when mask is NULL); nothing
 *        else is written, rows of unmasked envs are left as they are.  act / act8 may be NULL.
 * RS_ERR_INVALID_ARG, before anything is launched: NULL actors / critics / x / logp_val_boot, num_agents outside 1..RS_MAX_AGENTS,
 * num_envs < 1, a step round with NULL act.  The layouts are the ones rs_store_rows reads. */
int rs_ff_team_step(const rs_mlp_params* actors, const rs_mlp_params* critics, int32_t num_agents, const float* x, const float* u,
                    int64_t* act, float* logp_val_boot, int8_t* act8, const uint8_t* mask, int32_t num_envs, rs_stream_t stream);

/* ---- fused on-device collector ------------------------------------------------------------------
 * One launch = one epoch of the reference's collector loop (algos/multiagent/train.py:332-548) for all N
 * envs of the handle (single agent, N % 64 == 0, geom_group_size == 1): per lock-step the MLP forward on the
 * matrix cores, Philox inverse-CDF action sampling, the env step, the per-episode Welford standardisation
 * (RADTEAM_core.py:188-277, train.py:334-341,432-436), episode/epoch cut rules (train.py:394-405), the
 * bootstrap value (train.py:462-487), the masked reset (train.py:530) and the buffer row (PPOBuffer.store,
 * ppo.py:339-381).  Nothing leaves HBM; the policy weights are read once per launch. */
typedef struct rs_rollout_args {
    int32_t steps_per_epoch;    /* T */
    int32_t steps_per_episode;  /* L */
    /* rollout buffer, time-major (device, caller-owned) */
    float* obs;        /* [T,N,11] standardised observation fed to the networks */
    int64_t* act;      /* [T,N] */
    float* logp;       /* [T,N] */
    float* val;        /* [T,N] */
    float* rew;        /* [T,N] */
    float* last_val;   /* [T,N] bootstrap value where cut != 0 */
    uint8_t* cut;      /* [T,N] 1 = trajectory ends after this step */
    float* source_tar; /* [T,N,2] */
    /* collector state carried from epoch to epoch (device, caller-owned, [N]) */
    float* cur_obs;    /* [N,11] raw observation of the current state (from rs_reset / previous launch) */
    double* w_count;   /* Welford count, mean, M2, std */
    double* w_mean;
    double* w_sq;
    double* w_std;
    int32_t* steps_in_ep;
    float* ep_ret;
    /* per-env epoch statistics written by the launch ([N]) */
    int32_t* done_count;
    int32_t* oob_count;
    double* ep_ret_sum;
    double* ep_len_sum;
    int32_t* ep_count;
    /* per-env statistics of the returns of the episodes that ended in this launch (logger columns StdEpRet / MaxEpRet /
     * MinEpRet, train.py:620): sum of squares, max (-inf when none ended), min (+inf when none ended) */
    double* ep_ret_sq_sum;
    float* ep_ret_max;
    float* ep_ret_min;
} rs_rollout_args;

int rs_rollout(rs_handle* h, const rs_mlp_params* actor, const rs_mlp_params* critic, const rs_rollout_args* args,
               rs_stream_t stream);
/* the dynamic LDS bytes rs_rollout gives a workgroup of its kernel (has_obs != 0: the obstacle template); no device needed */
size_t rs_rollout_lds_bytes(int has_obs);

/* ---- fused PPO loss + gradients ------------------------------------------------------------------
 * One pass over the whole batch (M samples) computes the loss of AgentPPO.update_rada2c
 * (algos/multiagent/ppo.py:1206-1225) in its batched form
 *     L = -( sum_i w_i min(r_i A_i, clip(r_i, 1-c, 1+c) A_i)  -  vf * sum_i w_i (V_i - R_i)^2  +  alpha * sum_i w_i H_i )
 * (w_i = 1 / (#ranks * #episodes of the sample's rank * length of its episode): the reference's mean over
 * ranks of the mean over episodes of per-episode means; H_i enters as a DETACHED scalar exactly as in the
 * reference, `ent = pi.entropy().detach().mean().item()` ppo.py:1216, so alpha moves the loss value but
 * contributes no gradient), its statistics, and dL/dtheta for every parameter of
 * the actor and the critic: forward, loss, backward and the weight-gradient GEMMs (contraction over samples,
 * operands transposed through LDS) all on the matrix cores, gradients reduced deterministically.
 * Replaces loss_pi.backward() (ppo.py:1253-1254) for the FF_core networks.
 *   grads: float32 [10441] = actor {w1 704, b1 64, w2 4096, b2 64, w3 512, b3 8} then critic {704, 64, 4096, 64, 64, 1}
 *   stats: float64 [5] = {approx_kl, entropy, clip fraction, value loss, total loss}   (weighted sums)
 *   workspace: device scratch of rs_ppo_grad_workspace_bytes() bytes. */
typedef struct rs_ppo_batch {
    const float* x;        /* [M,11] */
    const int64_t* act;    /* [M] */
    const float* adv;      /* [M] normalised advantages */
    const float* ret;      /* [M] */
    const float* logp_old; /* [M] */
    const float* w;        /* [M] */
    int32_t M;
    float clip_ratio, alpha, vf_coef;
} rs_ppo_batch;

size_t rs_ppo_grad_workspace_bytes(void);
/* stop_flag (device int32, may be NULL): when non-zero at launch the call is a no-op (early stop already hit).
 * grads: float32 [RS_PPO_GRAD_FLOATS] = the 10441 gradients (actor w1 b1 w2 b2 w3 b3, critic ...) followed by the five
 * statistics once more as float32 (hi, lo) pairs (stats[q] = hi + lo) and zero padding: under data parallelism ONE
 * all-reduce (SUM) of this buffer is the reference's mpi_avg_grads + mpi_avg(kl) (ppo.py:1250-1256). */
#define RS_PPO_STATS_TAIL 16
#define RS_PPO_GRAD_FLOATS (10441 + RS_PPO_STATS_TAIL)
int rs_ppo_grad(const rs_mlp_params* actor, const rs_mlp_params* critic, const rs_ppo_batch* batch, float* grads,
                double* stats, void* workspace, const int32_t* stop_flag, rs_stream_t stream);

/* Device-side state of one update_agent call (algos/multiagent/ppo.py:789-796): lives in HBM so the whole
 * "<= train_pi_iters Adam steps with KL early stop" loop can be enqueued without a host round trip. */
typedef struct rs_update_state {
    int32_t adam_step;   /* optimiser step count (bias correction), persists across epochs            */
    int32_t stopped;     /* 1 once approx_kl >= threshold was seen in this update (reset by the host)  */
    int32_t iters;       /* loss evaluations done in this update == the reference's `kk`               */
    int32_t pad;
    double last_stats[5]; /* stats of the last evaluated iteration {kl, entropy, clipfrac, vloss, loss} */
} rs_update_state;

/* One iteration of the reference's early-stopped loop (ppo.py:1250-1261) after rs_ppo_grad:
 *   if state->stopped: nothing.  else iters += 1, last_stats = stats;
 *   if stats[0] (approx_kl, already reduced over ranks) < kl_threshold: Adam step (torch.optim.Adam
 *   semantics, betas (0.9, 0.999), eps 1e-8) on all 12 tensors with `grads`; else stopped = 1.
 * actor/critic point at the LIVE parameter tensors (updated in place); m, v: float32 [10441].
 * stats == NULL: take the statistics from the (hi, lo) pairs behind the gradients (the all-reduced bucket). */
int rs_adam_step(const rs_mlp_params* actor, const rs_mlp_params* critic, const float* grads, float* m, float* v,
                 const double* stats, rs_update_state* state, float lr, float kl_threshold, rs_stream_t stream);

/* rs_ppo_grad (with stop_flag = &state->stopped) followed by rs_adam_step (with its stats), for ONE rank: the slab reduction, the
 * Adam step and the state update run as one launch instead of three, behind ONE launch that runs the gradient passes of both networks
 * (environment RS_PPO_SPLIT_GRAD=1: one launch per network as in rs_ppo_grad, for A/B timing; same bits).  Every output -- grads
 * (with the (hi, lo) tail), stats, the parameters, m, v, *state -- is bitwise what the two calls leave.  Under data parallelism
 * an all-reduce of `grads` belongs between the two calls: use them. */
int rs_ppo_update_step(const rs_mlp_params* actor, const rs_mlp_params* critic, const rs_ppo_batch* batch, float* grads,
                       double* stats, void* workspace, float* m, float* v, rs_update_state* state, float lr, float kl_threshold,
                       rs_stream_t stream);

/* ---- RAD-TEAM heat maps (MapsBuffer, NeuralNetworkCores/RADTEAM_core.py:395-932) ------------------------
 * Per env the maps every agent's MapsBuffer would hold are kept ONCE (all owners see the same observations, so
 * readings / visit counts / obstacles / combined-locations maps and the estimator state are identical across
 * owners); the per-owner location map is a one-hot at the owner's cell and others = combined - location.
 *   rs_maps_update  <- MapsBuffer.observation_to_map (:532-616) for every env (one call per select_action round)
 *   rs_maps_reset   <- MapsBuffer.reset (:510-523) for the masked envs
 *   rs_maps_stack   <- CNNBase.get_map_stack (:1791-1836): actor [N,A,6,X,Y] = {prediction, location, others,
 *                      readings, visits, obstacles}, critic [N,4,X,Y] = {combined, readings, visits, obstacles}
 * visit_table: float32 [(steps_per_episode+1)*A + 1], visit_table[c] = the reference's
 * normalize_incremental_logscale(current_value = 2c, base, 2) evaluated by the caller (host Python math.log). */
typedef struct rs_maps rs_maps;
/* bits of the per-env "err" field (rs_maps_field): set by rs_maps_update, sticky -- rs_maps_reset leaves them -- until the caller
 * clears the field.  The maps of a flagged env no longer equal the reference's. */
enum {
    RS_MAPERR_RING_FULL = 1,      /* more than steps_per_episode + 2 updates without a reset: the reading was dropped             */
    RS_MAPERR_VISIT_OVERFLOW = 2, /* a cell visited more than (steps_per_episode + 1) * A + 1 times: the last table entry is used */
    RS_MAPERR_OFF_MAP = 4         /* a detector cell outside [-X, X) x [-Y, Y) (the reference's numpy indexing raises IndexError):
                                     clamped to the nearest edge cell                                                             */
};
size_t rs_maps_state_bytes(int32_t num_envs, int32_t num_agents, int32_t steps_per_episode, int32_t map_x, int32_t map_y);
int rs_maps_create(int32_t num_envs, int32_t num_agents, int32_t steps_per_episode, int32_t map_x, int32_t map_y,
                   double resolution_accuracy, const float* visit_table, void* workspace, size_t workspace_bytes,
                   rs_stream_t stream, rs_maps** out);
void rs_maps_destroy(rs_maps* m);
int rs_maps_reset(rs_maps* m, const uint8_t* mask, rs_stream_t stream);
/* obs [N,A,11] float32 (the env's observation rows); mask [N] or NULL (all).  Detector cells come from the env handle's integer
 * coordinates (from the observation rows when the env was created with coord_noise).
 * pred [N,A,2] float32 or NULL: owner a's location prediction in scaled coordinates.  Its cell is int(pred * resolution_accuracy) per
 * axis (truncation towards zero), and a negative cell -k with k <= X (Y) is cell X - k (Y - k), as numpy indexes
 * prediction_map[p0][p1] (RADTEAM_core.py:765).  A prediction outside that range, a NaN or an infinity -- where the reference raises --
 * and pred == NULL leave the owner's last prediction cell as it was (-1, an empty channel, after a reset); no flag is set. */
int rs_maps_update(rs_maps* m, rs_handle* env, const float* obs, const float* pred, const uint8_t* mask, rs_stream_t stream);
int rs_maps_stack(rs_maps* m, float* actor_stack, float* critic_stack, rs_stream_t stream);
/* introspection for tests: "pred_cell","cell" ([N,A] int32), "combined","readings","visits","obstacles" ([N,X*Y] f32) */
int rs_maps_field(rs_maps* m, const char* name, void** dev_ptr, int32_t* elem_bytes, int32_t* rows, int32_t* cols);

/* ---- RAD-TEAM CNN trunk (NeuralNetworkCores/RADTEAM_core.py:962-1023 Actor, :1211-1271 Critic) ----------------
 * conv3x3(Cin->8, pad 1) - ReLU - maxpool 2x2/2 - conv3x3(8->16, pad 1) - ReLU - Flatten on 27x27 maps, forward and
 * weight-gradient backward, reading the resident shared maps directly (replaces actor[0:6] / critic[0:6] of the
 * nn.Sequential and their autograd for a whole batch; the three Linear layers after it stay library GEMMs).
 *   maps   [S][4][729] float32: combined, readings, visits, obstacles of each sample
 *   agent >= 0: actor input (6 channels, CNNBase.get_map_stack :1791-1836) = {one-hot(pcells[s][agent]) or empty when
 *               -1, one-hot(cells[s][agent]), combined - location, readings, visits, obstacles}; cells/pcells [S][A] int64
 *   agent  < 0: critic input (4 channels) = maps as they are; cells/pcells ignored
 *   w1 [8][Cin][3][3], b1 [8], w2 [16][8][3][3], b2 [16]: torch Conv2d layouts
 *   a2 [S][2704] (= Flatten of the ReLU'd conv2 output).  For training (all three non-NULL, or all NULL) the forward
 *   also writes what backward consumes: p1 [S][169][8] float32 pooled activations, amax [S][169][8] uint8 the winning
 *   pixel (0..3, row-major, first maximum) of each 2x2 pool window, relu_mask [S][169] uint16 bit c = (a2 channel c > 0).
 * Backward: da2 [S][2704] = dL/d(a2); slab [rs_cnn_trunk_slab_rows(S, Cin)][rs_cnn_trunk_slab_row(Cin)] receives
 * per-workgroup partial sums laid out {dW1 8*Cin*9 | db1 8 | dW2 1152 | db2 16}; the caller sums the rows.
 * wscratch: device scratch of rs_cnn_trunk_scratch_floats(Cin) floats (the weights re-laid-out for scalar loads).
 * rs_cnn_trunk_forward_grid (host only, for tests): the workgroup count rs_cnn_trunk_forward launches for num_samples images, three
 * images per workgroup round. */
int32_t rs_cnn_trunk_slab_row(int32_t in_channels);
int32_t rs_cnn_trunk_slab_rows(int64_t num_samples, int32_t in_channels);
int32_t rs_cnn_trunk_forward_grid(int64_t num_samples, int32_t in_channels);
int32_t rs_cnn_trunk_scratch_floats(int32_t in_channels);
int rs_cnn_trunk_forward(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                         int64_t num_samples, const float* w1, const float* b1, const float* w2, const float* b2, float* a2,
                         float* p1, uint8_t* amax, uint16_t* relu_mask, float* wscratch, rs_stream_t stream);
int rs_cnn_trunk_backward(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                          int64_t num_samples, const float* w2, const float* da2, const uint16_t* relu_mask, const float* p1,
                          const uint8_t* amax, float* slab, float* wscratch, rs_stream_t stream);

/* ---- PFGRU location predictor -------------------------------------------------------------
 * One forward step of `self.model(obs_tensor, hidden)` in CNNBase.select_action (algos/test_cnn/RADTEAM_core.py:1872-1879):
 * PFGRUCell.forward (:1586-1631) = GRU-style particle update with reparameterised noise (:1517-1530), observation
 * likelihood + log-softmax (:1633-1641), soft resampling (:1466-1515), weighted particle mean -> hid_obs MLP (:1574-1584),
 * for every (owner, env) at once: 40 particles x 24 hidden units.
 *   weights   [A][RS_PFGRU_WEIGHT_FLOATS]  per-owner packed parameters (layout: csrc/rs_pfgru.hip; packer: pfgru.py)
 *   obs       [N][A][11]   the owner's own row supplies (reading, x, y)
 *   h, p      [A][N][6][40][4] particles, QUAD-major (a set's 40 particles x 24 units as six [40] x float4 slabs: unit u of particle q at
 *             ((u / 4) * 40 + q) * 4 + u % 4 -- coalesced for one particle per lane), [A][N][40] log weights; read; written back when
 *             carry_hidden != 0 (mask[n] != 0)
 *   base_key  [A][N], episode [N], calls [N]   counters of the draw hash (documented RNG deviation: the reference draws
 *             from torch's global generator)
 *   pred      [N][A][2]    location prediction (scaled coordinates, >= 0: the reference's MLP ends in a ReLU); with a mask only the
 *             masked envs' rows are written (the bootstrap round of the collectors, train.py:462-480: the others are not evaluated) */
#define RS_PFGRU_PARTICLES 40
#define RS_PFGRU_HIDDEN 24
#define RS_PFGRU_WEIGHT_FLOATS 3472
int rs_pfgru_step(const float* weights, const float* obs, float* h, float* p, const int64_t* base_key, const int64_t* episode,
                  const int64_t* calls, const uint8_t* mask, int32_t carry_hidden, double alpha, float* pred, int32_t num_envs,
                  int32_t num_agents, rs_stream_t stream);
/* A whole no-grad pass over an episode-major batch in ONE call: grad_step's PFGRU loop over an episode (RADA2C_core.py:555-558) for E
 * episodes of one predictor.  Enqueues rs_pfgru_reset and then the time steps t < steps on `stream`, four per launch (carried particle
 * sets staying in registers inside a launch; the step counter of step t = calls[t][.]; results identical to one rs_pfgru_step per t), each
 * launch over the first alive[t] episodes of its first step (episodes sorted by descending length: the ones still running are a prefix;
 * an episode that ends inside a launch's group of steps reports only its own steps).  obs [steps][E][11], calls [steps][E], pred [steps][E][2], alive: HOST array [steps].  Exists so that the
 * ~120 launches of a pass cost one library call: the policy loop of update_rada2c issues 40 such passes per update. */
int rs_pfgru_pass(const float* weights, const float* obs, float* h, float* p, const int64_t* base_key, const int64_t* episode,
                  const int64_t* calls, double alpha, float* pred, const int32_t* alive, int32_t steps, int32_t episodes, rs_stream_t stream);
/* The same step with the draws supplied instead of hashed: eps [A][N][40][24] = the reparameterisation noise, idx [A][N][40] = the
 * resampling indices (what FloatTensor.normal_ / torch.multinomial returned in a recorded run of the reference, :1485-1530).  The
 * arithmetic is the product kernel's (one template, two instantiations); used to hold it to tests/golden/pfgru.npz directly.  h is
 * quad-major as in rs_pfgru_step; eps stays particle-major. */
int rs_pfgru_step_recorded(const float* weights, const float* obs, float* h, float* p, const float* eps, const int32_t* idx,
                           const uint8_t* mask, int32_t carry_hidden, double alpha, float* pred, int32_t num_envs, int32_t num_agents,
                           rs_stream_t stream);
/* reset_hidden (RADTEAM_core.py:2030-2033, PFGRUCell.init_hidden :1643-1652) for the envs with mask[n] != 0 (all when null):
 * h0 ~ U[0,1) from the draw hash (written in rs_pfgru_step's quad-major layout), p0 = log(1/40).  episode[] / calls[] must already count
 * the new episode. */
int rs_pfgru_reset(float* h, float* p, const int64_t* base_key, const int64_t* episode, const int64_t* calls, const uint8_t* mask,
                   int32_t num_envs, int32_t num_agents, rs_stream_t stream);

/* ---- The PFGRU location predictor at hidden widths H = 8, 16, .., 64 (csrc/rs_pfgru_sized.hip) --------------------------------
 * rs_pfgru_step / _pass / _step_recorded / _reset with the width as the last argument before the stream: 40 particles, 3 inputs,
 * alpha, tanh and the hid_obs head Linear(H, 24)-ReLU-Linear(24, 2)-ReLU as the reference fixes them, the same draw hash, the particle
 * sets quad-major [A][N][H / 4][40][4], eps [A][N][40][H].  rs_pfgru_sized_weight_floats(H): floats per owner of the packed weights
 * (layout: csrc/rs_pfgru_sized.hip; packer: pfgru.py: pack_sized_weights), 0 when unsupported.  A width that is not a multiple of 8 in
 * 8..64 returns RS_ERR_UNSUPPORTED, NULL pointers or bad counts (N < 1, A outside 1..RS_MAX_AGENTS, steps < 1, alive[] not a
 * descending prefix count) RS_ERR_INVALID_ARG, both before anything is launched.  rs_pfgru_sized_pass takes up to 8 steps per launch. */
int32_t rs_pfgru_sized_weight_floats(int32_t hidden);
int rs_pfgru_sized_step(const float* weights, const float* obs, float* h, float* p, const int64_t* base_key, const int64_t* episode,
                        const int64_t* calls, const uint8_t* mask, int32_t carry_hidden, double alpha, float* pred, int32_t num_envs,
                        int32_t num_agents, int32_t hidden, rs_stream_t stream);
int rs_pfgru_sized_pass(const float* weights, const float* obs, float* h, float* p, const int64_t* base_key, const int64_t* episode,
                        const int64_t* calls, double alpha, float* pred, const int32_t* alive, int32_t steps, int32_t episodes, int32_t hidden,
                        rs_stream_t stream);
int rs_pfgru_sized_step_recorded(const float* weights, const float* obs, float* h, float* p, const float* eps, const int32_t* idx,
                                 const uint8_t* mask, int32_t carry_hidden, double alpha, float* pred, int32_t num_envs, int32_t num_agents,
                                 int32_t hidden, rs_stream_t stream);
int rs_pfgru_sized_reset(float* h, float* p, const int64_t* base_key, const int64_t* episode, const int64_t* calls, const uint8_t* mask,
                         int32_t num_envs, int32_t num_agents, int32_t hidden, rs_stream_t stream);

/* All draws of one PFGRU training pass over an episode-major batch (the counter hash of rada2c.HashDraws: keys [E] int64):
 * h0 [E][40][24] initial particles (uniforms), eps [L][E][40][24] reparameterisation noise (standard normals), u [L][E][40]
 * resampling uniforms (float64).  Replaces torch.rand / FloatTensor.normal_ / torch.multinomial's generator in update_model
 * (algos/multiagent/ppo.py:1062-1079 via RADA2C_core.py:199-211,279-288) -- the documented RNG deviation. */
int rs_pfgru_draws(const int64_t* keys, int32_t episodes, int32_t steps, float* h0, float* eps, double* u, rs_stream_t stream);

/* One pass of AgentPPO.update_model's loss and its gradients (algos/multiagent/ppo.py:1062-1128 + loss.backward()): the PFGRU
 * unrolled through every episode of an episode-major batch, the loss
 *     total_e = l2w * sum_t bp_t |loc_t - tar_t|^2 + l1w * 10 * sum_t bp_t |loc_t - tar_t|_1 / n_e
 *             + elbo * (l2w * sum_{t,c} -log mean_p exp(-(part_tpc - tar_tc)^2 bp_t) + l1w * 10 * sum_{t,c} -log mean_p exp(-|.| bp_t)) / n_e
 * (n_e = 2 x the episode's length; loc = hid_obs(weighted particle mean), part = hid_obs of every resampled particle), and
 * d (w_ep[e] * total_e) / d parameters by back-propagation through time, resampling indices held constant as in autograd.
 *   weights [RS_PFGRU_TRAIN_WEIGHT_FLOATS]  packed parameters (layout: csrc/rs_pfgru_train.hip; packer: rada2c.py)
 *   obs [L][E][11] (columns 0..2 used), target [L][E][2], bp [L][E], lens [E] (1..L; steps beyond are never touched), w_ep [E]
 *   h0 / eps / u  the draws of rs_pfgru_draws; u may be NULL: idx[] is then INPUT -- the resampling indices to take (the ones
 *                 torch.multinomial returned in a recorded run of the reference, tests/golden/rada2c_core.npz)
 *   hs [L][E][6][40][4], ps [L][E][40], gates [L][E][24][40][4]  scratch (the resampled particle sets; the forward walk's gates z | r | n |
 *                 eps * softplus'(var), reloaded by the backward walk), idx [L][E][40] the resampling indices taken (output when u is given)
 *   loss [E] = w_ep[e] * total_e;  grads [E][RS_PFGRU_TRAIN_GRAD_FLOATS] = the episode's gradient slab:
 *   d[fc_z | fc_r] [48][28] (column 27 = bias) | d fc_n [48][28] | d hid_obs[0] [24][25] | d hid_obs[2] [2][25] | d fc_obs [28];
 *   the caller sums the slabs over the episodes. */
#define RS_PFGRU_TRAIN_WEIGHT_FLOATS 3680
#define RS_PFGRU_TRAIN_GRAD_FLOATS 3376
int rs_pfgru_train(const float* weights, const float* obs, const float* target, const float* bp, const int64_t* lens, const float* w_ep,
                   const float* h0, const float* eps, const double* u, float* hs, float* ps, float* gates, int32_t* idx, float* loss,
                   float* grads, int32_t steps, int32_t episodes, double alpha, double l2_weight, double l1_weight, double elbo_weight,
                   rs_stream_t stream);
/* The same pass with the draws of rs_pfgru_draws(keys, ...) evaluated INSIDE the forward walk instead of read from h0 / eps / u: same keys,
 * same counter hash, same arithmetic -- bit-identical loss, gradients and indices -- without the 104 bytes per particle-step the draws
 * launch writes and the walk reads back (8.2 GB per pass at 16 500 episodes; ABI version 4).  h0 [E][40][24]: scratch (the forward walk
 * leaves the initial particles there for the backward walk's last step). */
int rs_pfgru_train_keyed(const float* weights, const float* obs, const float* target, const float* bp, const int64_t* lens, const float* w_ep,
                         const int64_t* keys, float* h0, float* hs, float* ps, float* gates, int32_t* idx, float* loss, float* grads, int32_t steps,
                         int32_t episodes, double alpha, double l2_weight, double l1_weight, double elbo_weight, rs_stream_t stream);

/* ---- The PFGRU training pass at hidden widths H = 8, 16, .., 64 (csrc/rs_pfgru_sized_train.hip) -------------------------------
 * rs_pfgru_draws and rs_pfgru_train with the width as an argument: 40 particles, 3 inputs, tanh, hid_obs Linear(H, 24)-ReLU-
 * Linear(24, 2)-ReLU, the same loss, the same draw hash (key particle * 4096 + unit), resampling indices constant in the backward pass.
 *   rs_pfgru_sized_train_weight_floats(H) / _grad_floats(H): floats of the packed weights / of one episode's gradient slab (layouts:
 *   csrc/rs_pfgru_sized_train.hip; packer / unpacker: rada2c.py: pack_sized_train_weights / unpack_sized_train_grads); 0 for a width
 *   that is not a multiple of 8 in 8..64.
 *   rs_pfgru_sized_draws: h0 [E][40][H], eps [L][E][40][H], u [L][E][40] (float64).
 *   rs_pfgru_sized_train: obs [L][E][11], target [L][E][2], bp [L][E], lens [E] (1..L; steps beyond are never touched), w_ep [E] (an
 *   episode with w_ep == 0 gets an exactly zero slab row and loss), h0 / eps / u as above; u may be NULL: idx[] is then INPUT and left
 *   untouched.  Scratch: hs [L][E][40][H] (the resampled particle set after every step), ps [L][E][2][40] (log weights before / after
 *   the step's resampling), gates [L][E][4][40][H] (z | r | n | eps * softplus'(var)); idx [L][E][40] (output when u is given);
 *   loss [E] = w_ep[e] * total_e; grads [E][rs_pfgru_sized_train_grad_floats(H)], the caller sums the rows:
 *   d[fc_z | fc_r] [2H][H + 4] (column H + 3 = bias) | d fc_n [2H][H + 4] | d hid_obs[0] [24][H + 1] | d hid_obs[2] [2][25] |
 *   d fc_obs [H + 4] | padding to a multiple of 16 (zero).
 * Both entries return RS_ERR_INVALID_ARG before anything is launched for an unsupported width, a NULL required pointer, steps < 1 or
 * episodes < 0; episodes == 0 is a successful no-op. */
int32_t rs_pfgru_sized_train_weight_floats(int32_t hidden);
int32_t rs_pfgru_sized_train_grad_floats(int32_t hidden);
int rs_pfgru_sized_draws(const int64_t* keys, int32_t episodes, int32_t steps, int32_t hidden, float* h0, float* eps, double* u,
                         rs_stream_t stream);
int rs_pfgru_sized_train(const float* weights, const float* obs, const float* target, const float* bp, const int64_t* lens, const float* w_ep,
                         const float* h0, const float* eps, const double* u, float* hs, float* ps, float* gates, int32_t* idx, float* loss,
                         float* grads, int32_t steps, int32_t episodes, double alpha, double l2_weight, double l1_weight, double elbo_weight,
                         int32_t hidden, rs_stream_t stream);

/* ---- RAD-A2C GRU recurrence -----------------------------------------------------------------
 * The time loop of torch.nn.GRU(13, 24, 1) as SeqPt.forward / grad_step run it over whole episodes
 * (NeuralNetworkCores/RADA2C_core.py:377-381, :550-566) and of its back-propagation through time, for an episode-major batch
 * (one episode per lane).  Gate order r, z, n; gh = W_hh h + b_hh; n = tanh(gi_n + r * gh_n); h' = (1 - z) n + z h.
 *   rs_gru_forward : gi [L][E][72] (= X W_ih^T + b_ih, computed by the caller), h0 [E][24],
 *                    whh_t [24][80] (k-major W_hh^T, columns 72..79 zero), bhh [80] (b_hh, zero padded)
 *                    -> hs [L][E][24] (h_t), gates [L][E][96] = r | z | n | (W_hn h_{t-1} + b_hn)
 *   rs_gru_backward: dhs [L][E][24] = dL/dh_t from everything downstream, hs, gates, h0, whh [72][32] (W_hh, columns 24..31 zero)
 *                    -> dgi [L][E][72] = dL/d(gi), dgh [L][E][72] = dL/d(gh); the caller forms dW_ih = sum dgi^T x,
 *                       db_ih = sum dgi, dW_hh = sum dgh^T h_{t-1}, db_hh = sum dgh. */
#define RS_GRU_HIDDEN 24
int rs_gru_forward(const float* gi, const float* h0, const float* whh_t, const float* bhh, float* hs, float* gates, int32_t steps,
                   int32_t episodes, rs_stream_t stream);
int rs_gru_backward(const float* dhs, const float* hs, const float* gates, const float* h0, const float* whh, float* dgi, float* dgh,
                    int32_t steps, int32_t episodes, rs_stream_t stream);

/* One step of the RAD-A2C actor-critic behind the PFGRU, for every env (RNNModelActorCritic.step after the location prediction,
 * NeuralNetworkCores/RADA2C_core.py:528-548): h' = GRU(cat(x, loc), h) (SeqPt.forward :377-381), logits = Woms(h') (:363-366),
 * value = Valms(h') (:367-368), action by inverse CDF of softmax(logits) on the caller's uniform u (Categorical.sample :541-544 --
 * documented RNG deviation), logp = log_softmax(logits)[action].
 *   weights [RS_RNN_POLICY_WEIGHT_FLOATS]  packed parameters (layout: csrc/rs_rnn_policy.hip; packer: rada2c.py)
 *   x [N][11], loc [N][2], h [N][24];  u [N] (needed when act / logp are wanted)
 *   outputs, any may be NULL: h_out [N][24] (may alias h), logits [N][8], value [N], act [N] int64, logp [N] */
#define RS_RNN_POLICY_WEIGHT_FLOATS 5296
int rs_rnn_policy_step(const float* weights, const float* x, const float* loc, const float* h, const float* u, float* h_out,
                       float* logits, float* value, int64_t* act, float* logp, int32_t num_envs, rs_stream_t stream);
/* The same step reading agent a's rows straight out of the collectors' [N][A][.] tensors (x_stride / loc_stride / u_stride: floats
 * between consecutive envs' rows) and writing the action once more as int8 into rs_step's action row (act8 [N][act8_stride]);
 * mask [N] or NULL: only the envs with mask != 0 are evaluated (the bootstrap round of a lock-step: the others' outputs are untouched). */
int rs_rnn_policy_step_rows(const float* weights, const float* x, int32_t x_stride, const float* loc, int32_t loc_stride, const float* h,
                            const float* u, int32_t u_stride, float* h_out, float* value, int64_t* act, float* logp, int8_t* act8,
                            int32_t act8_stride, const uint8_t* mask, int32_t num_envs, rs_stream_t stream);

/* The heads of the RAD-A2C actor-critic, update_rada2c's per-sample loss (algos/multiagent/ppo.py:1191-1234: PPO-clip surrogate on
 * the policy head, vf_coef x squared error on the value head; the entropy term carries no gradient) and their back-propagation,
 * for `samples` (step, episode) rows behind the GRU:
 *   hs [S][24], act [S], adv [S], ret [S], logp_old [S], sample_weight [S] (w_ep / episode length; 0 on padded steps)
 *   -> dhs [S][24] = dL/dh (what rs_gru_backward takes), dfac [S][80] = d pre-tanh of the policy head [32] | of the value head [32]
 *      | d logits [8] | d value | zeros, tfac [S][64] = tanh outputs of the two heads: the caller forms the weight gradients
 *      (dW1 = dfac[:, :32]^T hs, dW2 = dfac[:, 64:72]^T tfac[:, :32], ...; biases = column sums of dfac);
 *      stats [ceil(S / 64)][8]: per-wave weighted sums of kl, entropy, clip fraction, value loss, surrogate, weight. */
int rs_a2c_heads_loss(const float* weights, const float* hs, const int64_t* act, const float* adv, const float* ret, const float* logp_old,
                      const float* sample_weight, float* dhs, float* dfac, float* tfac, float* stats, int64_t samples, double clip_ratio,
                      double vf_coef, rs_stream_t stream);

/* ---- RAD-A2C actor-critic at other widths (csrc/rs_rnn_sized.hip) ------------------------------------------------------------
 * The counterparts of rs_rnn_policy_step_rows, rs_gru_forward / _backward, rs_a2c_heads_loss and rs_gru_h0_reset for a GRU of
 * hid = 1..64 units and single-hidden-layer heads of pol, val = 2..64 units (11 observations + 2 location inputs, 8 actions).  Widths
 * outside these ranges return RS_ERR_UNSUPPORTED, NULL pointers or bad counts RS_ERR_INVALID_ARG, both before anything is launched.
 *   rs_rnn_sized_weight_floats(hid, pol, val): floats of the packed actor-critic (layout: csrc/rs_rnn_sized.hip; packer: rada2c.py),
 *       0 when unsupported.  rs_gru_sized_weight_floats(hid): floats of the packed W_hh / b_hh that the sequence kernels read;
 *       rs_gru_sized_gate_floats(hid): floats per (step, episode) of their gates buffer.
 *   rs_rnn_sized_step: as rs_rnn_policy_step_rows with the widths as arguments and logits [N][8] as one more optional output;
 *       h / h_out [N][hid] (h_out may alias h).  Rows of a plain [N][.] call have strides 11 / 2 / 1.
 *   rs_gru_sized_forward : gi [L][E][3 hid], h0 [E][hid] -> hs [L][E][hid], gates [L][E][rs_gru_sized_gate_floats(hid)]
 *   rs_gru_sized_backward: dhs [L][E][hid], hs, gates, h0 -> dgi [L][E][3 hid], dgh [L][E][3 hid] (the caller forms the weight
 *       gradients as for rs_gru_backward)
 *   rs_a2c_sized_heads_loss: as rs_a2c_heads_loss with hs / dhs [S][hid], dfac [S][P8 + V8 + 16] = d pre-tanh policy [P8] | value [V8]
 *       | d logits [8] | d value | zeros, tfac [S][P8 + V8] (P8, V8: pol, val rounded up to a multiple of 8)
 *   rs_gru_h0_reset_sized: rs_gru_h0_reset for h [A][N][hid]. */
int32_t rs_rnn_sized_weight_floats(int32_t hid, int32_t pol, int32_t val);
int32_t rs_gru_sized_weight_floats(int32_t hid);
int32_t rs_gru_sized_gate_floats(int32_t hid);
int rs_rnn_sized_step(const float* weights, int32_t hid, int32_t pol, int32_t val, const float* x, int32_t x_stride, const float* loc,
                      int32_t loc_stride, const float* h, const float* u, int32_t u_stride, float* h_out, float* logits, float* value,
                      int64_t* act, float* logp, int8_t* act8, int32_t act8_stride, const uint8_t* mask, int32_t num_envs, rs_stream_t stream);
int rs_gru_sized_forward(const float* gi, const float* h0, const float* weights, float* hs, float* gates, int32_t hid, int32_t steps,
                         int32_t episodes, rs_stream_t stream);
int rs_gru_sized_backward(const float* dhs, const float* hs, const float* gates, const float* h0, const float* weights, float* dgi, float* dgh,
                          int32_t hid, int32_t steps, int32_t episodes, rs_stream_t stream);
int rs_a2c_sized_heads_loss(const float* weights, int32_t hid, int32_t pol, int32_t val, const float* hs, const int64_t* act, const float* adv,
                            const float* ret, const float* logp_old, const float* sample_weight, float* dhs, float* dfac, float* tfac,
                            float* stats, int64_t samples, double clip_ratio, double vf_coef, rs_stream_t stream);
int rs_gru_h0_reset_sized(float* h, const int64_t* base_key, const int64_t* episodes_begun, const uint8_t* mask, double scale, int32_t hid,
                          int32_t num_envs, int32_t num_agents, rs_stream_t stream);

/* ---- RAD-A2C teams: one policy round of every agent in one launch (csrc/rs_rnn_policy.hip, csrc/rs_rnn_sized.hip) -------------------
 * rs_rnn_team_step (GRU 24, heads 32 / 32) and rs_rnn_sized_team_step (hid 1..64, pol / val 2..64): grid = (64-lane groups, agent),
 * each agent with its own weights on its own rows of the collectors' tensors.  Every output equals num_agents calls of
 * rs_rnn_policy_step_rows (rs_rnn_sized_step) on agent a's rows, h_out = h in the step round, bit for bit.
 *   weights [A]             host array of device pointers, copied into the launch's arguments (a captured graph holds them by value);
 *                           each to RS_RNN_POLICY_WEIGHT_FLOATS, or rs_rnn_sized_weight_floats(hid, pol, val), packed floats
 *   x [N][A][11], loc [N][A][2], h [A][N][hid], u [N][A] or NULL, mask [N] or NULL (NULL: every env)
 *   act [A][N] int64 or NULL, logp_val_boot [A][3][N] or NULL, act8 [N][A] or NULL
 * Step round (u != NULL), on the envs with mask != 0: agent a's h row is updated in place (a lane reads its row before it stores);
 *   act8 and act, each if given, receive #{j < 7 : cdf_j <= u}; logp_val_boot, if given, receives the log-softmax at the action in
 *   slot 0 and the value in slot 1 -- without it the value head is not evaluated (an evaluation's use).
 * Bootstrap round (u == NULL): slot 2 of logp_val_boot receives the value of the GRU's next state on the masked envs; h is not
 *   written, nor anything else.
 * A masked-out env writes nothing in either round; a wave without a live env leaves at once.
 * RS_ERR_INVALID_ARG, before anything is launched: NULL weights / x / loc / h, a NULL entry among the first num_agents weights,
 * num_agents outside 1..RS_MAX_AGENTS, num_envs < 1, a step round with neither act nor act8, a bootstrap round without
 * logp_val_boot.  rs_rnn_sized_team_step: RS_ERR_UNSUPPORTED for widths outside the ranges above, as rs_rnn_sized_step. */
int rs_rnn_team_step(const float* const* weights, int32_t num_agents, const float* x, const float* loc, float* h, const float* u, int64_t* act,
                     float* logp_val_boot, int8_t* act8, const uint8_t* mask, int32_t num_envs, rs_stream_t stream);
int rs_rnn_sized_team_step(const float* const* weights, int32_t num_agents, int32_t hid, int32_t pol, int32_t val, const float* x,
                           const float* loc, float* h, const float* u, int64_t* act, float* logp_val_boot, int8_t* act8, const uint8_t* mask,
                           int32_t num_envs, rs_stream_t stream);

/* The forward trunk as the collectors use it: rs_cnn_trunk_prepare re-arranges a network's convolution weights into wscratch
 * (rs_cnn_trunk_scratch_floats floats) once per epoch, rs_cnn_trunk_infer is then ONE launch per select_action round (a2 only). */
int rs_cnn_trunk_prepare(int32_t in_channels, const float* w1, const float* b1, const float* w2, const float* b2, float* wscratch,
                         rs_stream_t stream);
int rs_cnn_trunk_infer(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent, int64_t num_samples,
                       const float* wscratch, float* a2, rs_stream_t stream);

/* ---- The same trunk for square maps of any side 8 <= map_side (M) <= 256 (rs_cnn_sized.hip): the maps without enforced walls
 * (RADTEAM_core.py:1727-1738; 147 x 147 for 120-step episodes).  The contract of rs_cnn_trunk_* with M*M cells per plane and the pooled
 * side P = M / 2 (floor, as torch's max_pool2d: an odd M drops the last conv1 row and column):
 *   maps [S][4][M*M]; cells / pcells [S][A] flat cell indices (-1 = empty one-hot); w1 [8][Cin][3][3], b1 [8], w2 [16][8][3][3], b2 [16]
 *   read in their torch layouts (no prepare step, no weight scratch);
 *   a2 [S][16*P*P] in torch's Flatten order (c*P*P + y*P + x).  For training (all three non-NULL, or all NULL): p1 [S][P*P][8],
 *   amax [S][P*P][8] uint8 (0..3, row-major, first maximum), relu_mask [S][P*P] uint16.  rs_cnn_sized_infer = the forward without them.
 * Backward: da2 [S][16*P*P]; slab [slab_rows][rs_cnn_sized_slab_row(Cin)] with slab_rows >= rs_cnn_sized_slab_rows(S, M, Cin) receives
 * per-workgroup partial sums {dW1 8*Cin*9 | db1 8 | dW2 1152 | db2 16}; the caller sums the first rs_cnn_sized_slab_rows rows.  No
 * atomics: the result is bit-identical from one call to the next.
 * A side outside [8, 256] returns RS_ERR_UNSUPPORTED (the slab functions return 0).
 *
 * The occupancy-aware training passes (walls-off maps are mostly empty).  A unit is (image, tile of 16 x 16 pooled cells); its forward
 * window is the pixels [2 ty0 - 3, 2 ty0 + 35) x [2 tx0 - 3, 2 tx0 + 35) of the four planes, clipped to the map.  A unit is EMPTY when
 * every element of that window compares equal to 0.0f (a NaN does not, -0.0f does) and, for an actor, neither the owner's cell nor its
 * prediction cell (-1: none) lies in the window.
 *   rs_cnn_sized_tiles: units per image, 0 for a side outside [8, 256].
 *   rs_cnn_sized_occupancy: flags [S][tiles], bit 0 = the window holds an element != 0.0f.  One read of the maps; the stored maps of an
 *   update do not change, so once per update.  The owner's cells are not in the flag: they differ per agent, the trunk passes test them.
 *   rs_cnn_sized_forward_occ: the training forward (p1, amax, relu_mask required) with flags (NULL: RS_ERR_INVALID_ARG).  Every output of
 *   every unit is written and is bit-identical to rs_cnn_sized_forward's; an empty unit neither reads its window nor evaluates conv1
 *   (p1 = max(0 + b1, 0), amax = 0) and takes its conv2 outputs from one evaluation per place in the map (first / inner / last row x column).
 *   rs_cnn_sized_backward_occ: rs_cnn_sized_backward with flags; p1 must be the forward's.  The same slab layout and rows, no atomics (two
 *   calls write identical slabs).  An empty unit reads only its da2 / relu_mask halo: with dZ2 the gated da2 and c1 = max(0 + b1, 0),
 *   db2 += sum dZ2, dW2[co][ci][ky][kx] += c1[ci] S[co][ky][kx] (S: dZ2 summed over the tile's pixels whose tap neighbour is in the map),
 *   db1[ci] += [c1[ci] > 0] sum w2[co][ci][ky][kx] R[co][ky][kx] (R: the tile's dZ2 sums shifted by the tap), dW1 += 0.  The sums are
 *   reassociated: equal to rs_cnn_sized_backward to float32 summation order, not bit for bit. */
int32_t rs_cnn_sized_tiles(int32_t map_side);
int rs_cnn_sized_occupancy(const float* maps, int64_t num_samples, int32_t map_side, uint8_t* flags, rs_stream_t stream);
int rs_cnn_sized_forward_occ(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                             int64_t num_samples, int32_t map_side, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* a2, float* p1, uint8_t* amax, uint16_t* relu_mask, const uint8_t* flags, rs_stream_t stream);
int rs_cnn_sized_backward_occ(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                              int64_t num_samples, int32_t map_side, const float* w2, const float* da2, const uint16_t* relu_mask,
                              const float* p1, const uint8_t* amax, float* slab, int32_t slab_rows, const uint8_t* flags,
                              rs_stream_t stream);
int32_t rs_cnn_sized_slab_row(int32_t in_channels);
int32_t rs_cnn_sized_slab_rows(int64_t num_samples, int32_t map_side, int32_t in_channels);
int rs_cnn_sized_forward(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                         int64_t num_samples, int32_t map_side, const float* w1, const float* b1, const float* w2, const float* b2,
                         float* a2, float* p1, uint8_t* amax, uint16_t* relu_mask, rs_stream_t stream);
int rs_cnn_sized_infer(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent, int64_t num_samples,
                       int32_t map_side, const float* w1, const float* b1, const float* w2, const float* b2, float* a2, rs_stream_t stream);
int rs_cnn_sized_backward(const float* maps, const int64_t* cells, const int64_t* pcells, int32_t num_agents, int32_t agent,
                          int64_t num_samples, int32_t map_side, const float* w2, const float* da2, const uint16_t* relu_mask,
                          const float* p1, const uint8_t* amax, float* slab, int32_t slab_rows, rs_stream_t stream);

/* The RAD-TEAM heads behind their first Linear layer (CNNBase.select_action, RADTEAM_core.py:1838-1892; Actor :1000-1023, Critic
 * :1250-1271): y1 [N][32] = Linear(2704, 32)(a2), pre-activation -> ReLU -> Linear(32, 16) (w2 [16][32], b2) -> ReLU -> Linear(16, out_dim)
 * (w3 [out_dim][16], b3).  out_dim = 8: the action logits -> log-softmax, inverse-CDF draw on u [n * u_stride] (a = #{j < 7: cdf_j <= u}),
 * act [N] int64, logp [N], act8 [n * act8_stride] (any NULL: not written).  out_dim = 1: the state value, written value_copies times at
 * value_stride floats.  mask [N] or NULL: only those envs. */
int rs_cnn_head(const float* y1, const float* w2, const float* b2, const float* w3, const float* b3, int32_t out_dim, const float* u,
                int32_t u_stride, int64_t* act, float* logp, int8_t* act8, int32_t act8_stride, float* value, int32_t value_copies,
                int64_t value_stride, const uint8_t* mask, int32_t num_envs, rs_stream_t stream);

/* The PPO-clip actor loss of the RAD-TEAM update behind the logits (AgentPPO.compute_loss_pi, algos/multiagent/ppo.py:966-1003) and its
 * derivative, one pass: logits [S][8], act [S], adv [S], logp_old [S], sample_weight [S] ->
 *   dlogits [S][8] = d (-sum_s w_s min(ratio_s adv_s, clip(ratio_s) adv_s)) / d logits,
 *   stats [ceil(S / 64)][4]: per-wave weighted sums of kl (logp_old - logp), entropy, clip fraction and the loss itself. */
int rs_actor_loss(const float* logits, const int64_t* act, const float* adv, const float* logp_old, const float* sample_weight,
                  float* dlogits, float* stats, int64_t samples, double clip_ratio, rs_stream_t stream);

/* _get_init_states (RADA2C_core.py:458-461) for the envs with mask[n] != 0 (all when NULL): GRU state h [A][N][24] ~
 * U(-scale, scale), scale = 1 / sqrt(24), from the counter hash of the env's key base_key [A][N] and its episode counter
 * episodes_begun [N] (documented RNG deviation: the reference draws from torch's global generator). */
int rs_gru_h0_reset(float* h, const int64_t* base_key, const int64_t* episodes_begun, const uint8_t* mask, double scale, int32_t num_envs,
                    int32_t num_agents, rs_stream_t stream);

/* ---- running observation statistics ------------------------------------------------------------
 * StatisticStandardization.update / standardize / reset (NeuralNetworkCores/RADTEAM_core.py:188-277) for num_envs x num_agents
 * independent streams, float64 state count / mean / sq (square_dist_mean) / std, one pass each:
 *   update      : streams of the envs with mask[n] != 0 (all when NULL) take the reading reading[i * stride], i = n * A + a
 *                 (Welford; the first sample sets the mean only; std = max(sqrt(sq / (count - 1)), 1))
 *   reset       : count = mean = sq = 0, std = 1 for the masked envs
 *   standardize : out[i * out_stride] = (float)((reading[i * stride] - mean[i]) / std[i]) */
int rs_welford_update(double* count, double* mean, double* sq, double* std, const float* reading, int64_t stride, const uint8_t* mask,
                      int32_t num_envs, int32_t num_agents, rs_stream_t stream);
int rs_welford_reset(double* count, double* mean, double* sq, double* std, const uint8_t* mask, int32_t num_envs, int32_t num_agents,
                     rs_stream_t stream);
int rs_welford_standardize(const double* mean, const double* std, const float* reading, int64_t stride, float* out, int64_t out_stride,
                           int32_t streams, rs_stream_t stream);

/* The logger statistics train() accumulates per epoch and agent id (algos/multiagent/train.py:386-398, :494-501, :519-526), one
 * lock-step of all envs: acc_oob[a] += sum_n out_of_bounds[n][a]; acc_done[a] += sum_n done[n][a]; over the envs whose episode
 * ended (over[n] != 0): ep_cnt += 1, ep_len += steps_in_ep[n], ret_sum[a] += r, ret_sq[a] += r^2, ret_max / ret_min (r =
 * ep_ret[n][a]).  float64 accumulators, fixed summation order. */
int rs_epoch_stats(const uint8_t* out_of_bounds, const uint8_t* done, const float* ep_ret, const int32_t* steps_in_ep, const uint8_t* over,
                   double* acc_oob, double* acc_done, double* ep_cnt, double* ep_len, double* ret_sum, double* ret_sq, double* ret_max,
                   double* ret_min, int32_t num_envs, int32_t num_agents, rs_stream_t stream);

/* PPOBuffer.store (algos/multiagent/ppo.py:296-389) for one lock-step of every (env, agent): row *t (a device-side counter) of the
 * time-major rollout buffers receives act [A][N], logp / value / bootstrap value (logp_val_boot [A][3][N]; the bootstrap value only
 * where boot[n] != 0, else 0), the observation x [N][A][11], the source location (src_x, src_y [N] int32 -> float), the reward
 * rew [N][A] and the cut flag cut [N]. */
int rs_store_rows(const int64_t* t, const int64_t* act, const float* logp_val_boot, const float* x, const int32_t* src_x, const int32_t* src_y,
                  const float* rew, const uint8_t* cut, const uint8_t* boot, int64_t* buf_act, float* buf_logp, float* buf_val,
                  float* buf_last_val, float* buf_obs, float* buf_source, float* buf_rew, uint8_t* buf_cut, int32_t num_envs,
                  int32_t num_agents, int32_t steps_per_epoch, rs_stream_t stream);

/* The element-wise bookkeeping of one collector lock-step between the library calls -- the epoch loop body of train_PPO.train
 * (algos/multiagent/train.py:332-548) for all envs at once: what the reference does in Python per env and step, as three launches.
 * Every pointer is a device buffer of the caller (addresses fixed for the life of the collector: the lock-step is replayed as a graph).
 *   rs_collect_pre        x <- obs with the reading (column 0) standardised by the running statistics (:334-341)
 *   rs_collect_post_step  after rs_step: ep_ret += reward (the team reward for every agent when team_reward != 0, :366-375),
 *                         steps_in_ep += 1, over = any agent's terminal flag | steps_in_ep == steps_per_episode (:387-405),
 *                         cut = over (everything at the epoch's last step), boot = timeouts (all cut envs at the epoch's last step:
 *                         the envs whose value is bootstrapped, :462-487); Welford update with the new readings (:432-436);
 *                         obs <- env_obs; xb <- its standardised form; pf_calls += 1 (the predictor bank's per-env call counter)
 *   rs_collect_post_reset after rs_reset(cut): pf_calls += boot (the bootstrap round's prediction); for the cut envs obs <- env_obs,
 *                         ep_ret = 0, steps_in_ep = 0, statistics restarted on the first reading (:504-548) and, with reset_hidden,
 *                         pf_episode += 1, pf_calls = 0, episodes_begun += 1 (the draw counters rs_pfgru_reset / rs_gru_h0_reset read);
 *                         t += 1 */
typedef struct {
    int32_t num_envs, num_agents, steps_per_episode, team_reward;
    const float* env_obs;         /* [N][A][11] the env's observation rows (output of rs_step / rs_reset) */
    const float* env_reward;      /* [N][A] */
    const float* env_team;        /* [N] */
    const uint8_t* env_done;      /* [N][A] */
    float* obs;                   /* [N][A][11] the collector's current observation */
    float* ep_ret;                /* [N][A] */
    int32_t* steps_in_ep;         /* [N] */
    double* w_count; double* w_mean; double* w_sq; double* w_std;     /* [N][A] Welford state of the readings; all NULL: no standardisation */
    float* x;                     /* [N][A][11] policy input of the step (rs_collect_pre); may be NULL for post_step / post_reset */
    float* xb;                    /* [N][A][11] policy input of the bootstrap round, or NULL */
    float* reward_used;           /* [N][A] or NULL */
    uint8_t* over; uint8_t* cut; uint8_t* boot;                        /* [N] */
    int64_t* pf_episode; int64_t* pf_calls; int64_t* episodes_begun;   /* [N] or NULL */
    int64_t* t;                   /* [1] device-side step counter, or NULL */
    /* copies of what rs_store_rows / rs_epoch_stats read of the env's output rows, taken by rs_collect_post_step so that rs_reset (which
     * rewrites those rows and moves the sources of the cut envs) may run beside the bootstrap round on another stream; all or none NULL */
    const uint8_t* env_oob;       /* [N][A] info.out_of_bounds */
    const int32_t* env_src_x; const int32_t* env_src_y;               /* [N] */
    uint8_t* done_copy; uint8_t* oob_copy;                            /* [N][A] */
    int32_t* src_copy;            /* [2][N] */
    int64_t* complete_len;        /* [N] or NULL: t + 1 of the env's last episode end so far in the epoch (what sample() of the 'cnn' update
                                   * counts, algos/multiagent/ppo.py:754-764); set by rs_collect_post_step where over != 0 */
} rs_collect_state;
int rs_collect_pre(const rs_collect_state* c, rs_stream_t stream);
int rs_collect_post_step(const rs_collect_state* c, int32_t epoch_ended, rs_stream_t stream);
int rs_collect_post_reset(const rs_collect_state* c, int32_t reset_hidden, rs_stream_t stream);

/* ---- Monte-Carlo evaluation of feed-forward agents and teams (algos/multiagent/evaluate.py:355-475) --------------------------------
 * One evaluation lock-step is rs_action_uniforms, rs_ff_eval_step, rs_step, rs_eval_post_step on one stream
 * (radiation_ppo_amd/evaluate.py: run_test_environments_team); a lane is one (saved environment, Monte-Carlo run) pair.
 *
 * rs_ff_eval_step: the policy round for every agent of the team in one launch, grid = (64-sample groups, agent); forward pass and
 * sampler are rs_ff_team_step's, the critic is not evaluated.
 *   actors [A]            host array of rs_mlp_params (device pointers inside), A = num_agents in 1..RS_MAX_AGENTS
 *   obs [N][A][11]        the raw current observation
 *   w_mean, w_std [N][A]  float64 running statistics of the reading (DeviceWelford's layout): element 0 of a row enters the network as
 *                         (float)(((double)obs0 - mean) / std), rs_welford_standardize's expression; both NULL: no standardisation
 *   u [N][A], alive [N]   the uniforms of rs_action_uniforms; alive[n] != 0 while lane n's episode runs
 *   act8 [N][A]           rs_step's action rows: #{j < 7 : cdf_j <= u} where alive, else 8 (idle)
 * RS_ERR_INVALID_ARG, before anything is launched: NULL actors / obs / u / alive / act8, exactly one of w_mean / w_std NULL,
 * num_agents outside 1..RS_MAX_AGENTS, num_envs < 1. */
int rs_ff_eval_step(const rs_mlp_params* actors, int32_t num_agents, const float* obs, const double* w_mean, const double* w_std,
                    const float* u, const uint8_t* alive, int8_t* act8, int32_t num_envs, rs_stream_t stream);

/* rs_eval_post_step: everything between rs_step and the next policy round, one launch, one thread per lane, in this order:
 *   r = use_team_reward ? env_team[n] : env_reward[n][0] (`episode_return[0]`, evaluate.py:400-447); where alive: ep_ret += r (float32),
 *   ep_len += 1; found = alive and any agent's env_done; success |= found, alive &= !found; where still alive the Welford update of
 *   rs_welford_update on every agent's new reading; cur_obs <- env_obs on every lane; finished[0] += the lanes that stopped in this
 *   launch (a monotonic counter: the host reads it once every few lock-steps and never zeroes it inside the loop).
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL struct or required field, A outside 1..RS_MAX_AGENTS, N < 1, some but not
 * all of the four Welford pointers. */
typedef struct {
    int32_t N, A, use_team_reward;
    const float* env_obs;         /* [N][A][11] the env's output rows (rs_step) */
    const float* env_reward;      /* [N][A] */
    const float* env_team;        /* [N] */
    const uint8_t* env_done;      /* [N][A] */
    float* cur_obs;               /* [N][A][11] the observation the next policy round reads */
    double* w_count; double* w_mean; double* w_sq; double* w_std;     /* [N][A] Welford state of the readings; all NULL: none kept */
    uint8_t* alive; uint8_t* success;                                 /* [N] */
    int32_t* ep_len;              /* [N] */
    float* ep_ret;                /* [N] */
    int32_t* finished;            /* [1] */
} rs_eval_state;
int rs_eval_post_step(const rs_eval_state* s, rs_stream_t stream);

/* ---- Monte-Carlo evaluation of the recurrent agent, RAD-A2C (algos/multiagent/evaluate.py:333-476) -----------------------------------
 * A lane is one agent (A = 1) working through runs_per_lane consecutive runs of one saved environment: runs_per_lane = R on N = E lanes
 * keeps the reference's hidden-state lifetime (`hiddens` is created once per EpisodeRunner.run, :357), runs_per_lane = 1 on N = E R
 * lanes gives every run a lane of its own.  One lock-step is rs_action_uniforms, rs_pfgru_step (mask = active), rs_rnn_policy_step_rows
 * or rs_rnn_sized_step (mask = active, act8 = the step's action row), rs_step, rs_rnn_eval_post_step and, when runs_per_lane > 1,
 * rs_refresh(mask = again) and rs_rnn_eval_post_refresh, all on one stream.
 * This section is the A = 1 case of the team section below it: rs_rnn_eval_state is rs_rnn_team_eval_state without the field A, and the
 * two entries widen it on the host and launch the team's kernels, with the team entries' refusals.  The package's own runners
 * (radiation_ppo_amd/evaluate.py: run_test_environments_rnn, a front to run_test_environments_rnn_team) use the team entries.
 *
 * rs_rnn_eval_post_step: one launch after rs_step, one thread per lane, in this order (a = active[n] on entry):
 *   where a: ret += env_reward (float32), steps += 1, pf_calls += 1; found = a and env_done, over = found or (a and steps ==
 *   steps_per_episode); where a: the Welford update of rs_welford_update with env_obs[n][0] (before the episode-over test, :392-397;
 *   the first sample sets the mean only); where over: rec_len / rec_ret / rec_suc [n][run] = steps, ret, found, then run += 1,
 *   steps = 0, ret = 0; again = over and run < runs_per_lane; where over and run == runs_per_lane: active = 0, idle_act8[n] = 8 and
 *   the lane counts once into finished[0] (a monotonic counter: the host reads it once every few lock-steps and never zeroes it inside
 *   the loop); on every lane cur_obs <- env_obs and x <- env_obs with x[0] = (float)(((double)obs0 - mean) / std), the statistics as
 *   just updated (rs_welford_standardize's expression).
 * rs_rnn_eval_post_refresh: one launch after rs_refresh(mask = again), which rewrites the env rows of those lanes only.  Where
 *   again != 0: the statistics restart (count = mean = sq = 0, std = 1) and take the refreshed reading as their first sample,
 *   cur_obs <- env_obs, x <- its standardised form (:455-468).  The other lanes are untouched, and so are all hidden states.
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL struct or required field, N < 1, runs_per_lane < 1, steps_per_episode < 1.
 * Only pf_calls and idle_act8 may be NULL. */
typedef struct {
    int32_t N, runs_per_lane, steps_per_episode;
    const float* env_obs;         /* [N][11] the env's output rows (rs_step / rs_refresh) */
    const float* env_reward;      /* [N] */
    const uint8_t* env_done;      /* [N] */
    float* cur_obs;               /* [N][11] the current observation */
    float* x;                     /* [N][11] the PFGRU's and the policy's input: cur_obs with the reading standardised */
    double* w_count; double* w_mean; double* w_sq; double* w_std;     /* [N] Welford state of the reading; all required */
    uint8_t* active;              /* [N] != 0 while the lane has runs left */
    uint8_t* again;               /* [N] written by rs_rnn_eval_post_step, read by rs_refresh (its mask) and rs_rnn_eval_post_refresh */
    int32_t* run; int32_t* steps; /* [N] index of the current run, steps taken in it */
    float* ret;                   /* [N] its return so far */
    int32_t* rec_len; float* rec_ret; uint8_t* rec_suc;               /* [N][runs_per_lane] the records of the runs that ended */
    int64_t* pf_calls;            /* [N] or NULL: the predictor bank's per-lane call counter */
    int8_t* idle_act8;            /* [N] or NULL: rs_step's action row where one fixed buffer serves every lock-step */
    int32_t* finished;            /* [1] lanes whose last run has ended */
} rs_rnn_eval_state;
int rs_rnn_eval_post_step(const rs_rnn_eval_state* s, rs_stream_t stream);
int rs_rnn_eval_post_refresh(const rs_rnn_eval_state* s, rs_stream_t stream);

/* ---- Monte-Carlo evaluation of RAD-A2C teams of 2 to 8 recurrent agents (algos/multiagent/evaluate.py:305-318, :333-476) -------------
 * Every agent has its own network (:305-318), its own `hiddens` entry, created once per EpisodeRunner.run (:353), and its own statistics
 * buffer (:361-364, :395-397, :461-466); an episode ends when any agent's terminal flag rises (:411-423) or at steps_per_episode, and
 * agent 0's return is recorded (`episode_return[0]`, :441-444).  A lane is one team working through runs_per_lane consecutive runs of one
 * saved environment, as for the single agent above.  One lock-step is rs_action_uniforms, rs_pfgru_step (every owner, mask = active),
 * rs_rnn_team_eval_step (or, at other widths, rs_rnn_sized_team_step without act and logp_val_boot), rs_step, rs_rnn_team_eval_post_step and,
 * when runs_per_lane > 1, rs_refresh(mask = again) and rs_rnn_team_eval_post_refresh, all on one stream
 * (radiation_ppo_amd/evaluate.py: run_test_environments_rnn_team).
 *
 * rs_rnn_team_eval_step: the policy round of every agent of a default-width team (GRU 24, heads 32 / 32) in one launch,
 * grid = (64-lane groups, agent); the arithmetic is rs_rnn_policy_step_rows', operation by operation, without the value head: the
 * result equals num_agents calls of rs_rnn_policy_step_rows (mask = active, h_out = h) bit for bit.
 *   weights [A]           host array of device pointers, each to RS_RNN_POLICY_WEIGHT_FLOATS packed floats, A = num_agents
 *   x [N][A][11]          the standardised observation
 *   loc [N][A][2]         the location predictions (rs_pfgru_step's pred)
 *   h [A][N][24]          the GRU states, updated in place on the active lanes (a lane reads its row before it stores)
 *   u [N][A], active [N]  the uniforms of rs_action_uniforms; active[n] != 0 while lane n has runs left
 *   act8 [N][A]           rs_step's action rows: #{j < 7 : cdf_j <= u} on the active lanes
 * An inactive lane writes neither h nor act8; a wave without an active lane leaves at once.
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL pointer, a NULL entry among the first num_agents weights, num_agents outside
 * 1..RS_MAX_AGENTS, num_envs < 1. */
int rs_rnn_team_eval_step(const float* const* weights, int32_t num_agents, const float* x, const float* loc, float* h, const float* u,
                          const uint8_t* active, int8_t* act8, int32_t num_envs, rs_stream_t stream);

/* rs_rnn_team_eval_post_step: one launch after rs_step, one thread per lane, in this order (a = active[n] on entry):
 *   where a: ret += env_reward[n][0] (float32), steps += 1, pf_calls += 1 (the bank keeps one counter per lane, not one per owner);
 *   found = a and any agent's env_done[n][.], over = found or (a and steps == steps_per_episode); where a: every agent's statistics take
 *   env_obs[n][agent][0] (the Welford update of rs_welford_update, before the episode-over test, :395-397); where over: rec_len /
 *   rec_ret / rec_suc [n][run] = steps, ret, found, then run += 1, steps = 0, ret = 0; again = over and run < runs_per_lane; where
 *   over and run == runs_per_lane: active = 0, all A entries of idle_act8[n] = 8 and the lane counts once into finished[0] (a monotonic
 *   counter); on every lane cur_obs <- env_obs and x <- env_obs with x[n][agent][0] = (float)(((double)obs0 - mean) / std), that
 *   agent's statistics as just updated.
 * rs_rnn_team_eval_post_refresh: one launch after rs_refresh(mask = again).  Where again != 0: every agent's statistics restart
 *   (count = mean = sq = 0, std = 1) and take the refreshed reading as their first sample, cur_obs <- env_obs, x <- its standardised
 *   form (:456-466).  The other lanes are untouched, and so are all hidden states.
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL struct or required field, A outside 1..RS_MAX_AGENTS, N < 1,
 * runs_per_lane < 1, steps_per_episode < 1.  Only pf_calls and idle_act8 may be NULL. */
typedef struct {
    int32_t N, A, runs_per_lane, steps_per_episode;
    const float* env_obs;         /* [N][A][11] the env's output rows (rs_step / rs_refresh) */
    const float* env_reward;      /* [N][A] */
    const uint8_t* env_done;      /* [N][A] */
    float* cur_obs;               /* [N][A][11] the current observation */
    float* x;                     /* [N][A][11] the PFGRUs' and the policies' input: cur_obs with the readings standardised */
    double* w_count; double* w_mean; double* w_sq; double* w_std;     /* [N][A] Welford state of the readings; all required */
    uint8_t* active;              /* [N] != 0 while the lane has runs left */
    uint8_t* again;               /* [N] written by the post-step, read by rs_refresh (its mask) and the post-refresh */
    int32_t* run; int32_t* steps; /* [N] index of the current run, steps taken in it */
    float* ret;                   /* [N] agent 0's return so far */
    int32_t* rec_len; float* rec_ret; uint8_t* rec_suc;               /* [N][runs_per_lane] the records of the runs that ended */
    int64_t* pf_calls;            /* [N] or NULL: the predictor bank's per-lane call counter */
    int8_t* idle_act8;            /* [N][A] or NULL: rs_step's action rows where one fixed buffer serves every lock-step */
    int32_t* finished;            /* [1] lanes whose last run has ended */
} rs_rnn_team_eval_state;
int rs_rnn_team_eval_post_step(const rs_rnn_team_eval_state* s, rs_stream_t stream);
int rs_rnn_team_eval_post_refresh(const rs_rnn_team_eval_state* s, rs_stream_t stream);

/* ---- Monte-Carlo evaluation of RAD-TEAM (CNN) teams of 1 to 8 agents on 27 x 27 maps (algos/multiagent/evaluate.py:333-476) ---------
 * One lock-step is rs_action_uniforms, rs_pfgru_step (every owner), rs_maps_update, rs_maps_stack, rs_cnn_team_trunk_infer,
 * rs_cnn_team_eval_head, rs_step, rs_eval_post_step (its four Welford pointers NULL) on one stream
 * (radiation_ppo_amd/evaluate.py: run_test_environments_cnn_team); every agent's convolution weights are prepared once per run, one
 * rs_cnn_trunk_prepare(6, ...) per agent into wscratch [A][rs_cnn_trunk_scratch_floats(6)].
 *
 * rs_cnn_team_trunk_infer: every agent's actor trunk in one launch, grid = (image rounds, agent); the arithmetic is rs_cnn_trunk_infer's:
 * the result equals num_agents calls of it (agent = a, a's prepared weights) bit for bit.
 *   maps [N][4][729]          the shared maps (rs_maps_stack's critic stack)
 *   cells, pcells [N][A]      int32: the heat maps' own "cell" / "pred_cell" fields (rs_maps_field), -1 = none
 *   wscratch [A][scratch]     the prepared weights, scratch = rs_cnn_trunk_scratch_floats(6)
 *   a2 [A][N][2704]           every agent's flattened trunk output
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL pointer, num_agents outside 1..RS_MAX_AGENTS, num_samples < 0;
 * num_samples == 0 returns RS_OK and launches nothing. */
int rs_cnn_team_trunk_infer(const float* maps, const int32_t* cells, const int32_t* pcells, int32_t num_agents, int64_t num_samples,
                            const float* wscratch, float* a2, rs_stream_t stream);

/* rs_cnn_team_eval_head: every agent's policy head behind the trunk in one launch, grid = (64-image tiles, agent): Linear(2704, 32) on
 * the f32 matrix cores (exact f32; four k-quarters added in a fixed order, then the bias: no atomics, an image's bits depend on neither
 * num_envs nor the grid), then rs_cnn_head's arithmetic (out_dim 8) operation for operation and the evaluation's idle rule.
 *   heads [A]             host array (device pointers inside), torch layouts: w1 [32][2704], b1 [32], w2 [16][32], b2 [16], w3 [8][16], b3 [8]
 *   a2 [A][N][2704]       rs_cnn_team_trunk_infer's output
 *   u [N][A], alive [N]   the uniforms of rs_action_uniforms; alive[n] != 0 while lane n's episode runs
 *   act8 [N][A]           rs_step's action rows: #{j < 7 : cdf_j <= u} where alive, else 8 (idle)
 *   act [A][N], logp [A][N], y1_out [A][N][32]   or NULL: the draw and its log-probability on EVERY lane, alive or not, and the first
 *                         layer's pre-activation output (for tests; the evaluation passes NULL)
 * RS_ERR_INVALID_ARG, before anything is launched: NULL heads / a2 / u / alive / act8, a NULL pointer inside the first num_agents heads,
 * num_agents outside 1..RS_MAX_AGENTS, num_envs < 1. */
typedef struct { const float *w1, *b1, *w2, *b2, *w3, *b3; } rs_cnn_head_params;
int rs_cnn_team_eval_head(const rs_cnn_head_params* heads, int32_t num_agents, const float* a2, const float* u, const uint8_t* alive,
                          int8_t* act8, int64_t* act, float* logp, float* y1_out, int32_t num_envs, rs_stream_t stream);

/* ---- The same evaluation for square maps of any side 8 <= map_side (M) <= 256: the maps without enforced walls, 147 x 147 for 120-step
 * episodes (radiation_ppo_amd/evaluate.py: run_test_environments_cnn_team_sized).  One lock-step is rs_action_uniforms, rs_pfgru_step
 * (every owner), rs_maps_update, rs_maps_stack, then per chunk of lanes rs_cnn_sized_team_infer and rs_cnn_sized_team_eval_head (the
 * chunk bounds the a2 scratch: 16 P P floats per lane and agent, P = M / 2), rs_step, rs_eval_post_step on one stream.
 *
 * rs_cnn_sized_team_infer: every agent's actor trunk in one launch of the tiled trunk (rs_cnn_sized.hip), a persistent grid over the
 * (agent, image, tile) units; the arithmetic is rs_cnn_sized_infer's: the result equals num_agents calls of it (agent = a, a's weights)
 * bit for bit.  A unit whose staged 38 x 38 x 4 input window holds nothing but zeros (every element == 0.0f) and neither of the agent's
 * two cells does not evaluate conv1: its pooled cells are max(0 + b1, 0), which is what conv1 gives there, bit for bit.
 *   maps [S][4][M*M]          the shared maps (rs_maps_stack's critic stack)
 *   cells, pcells [S][A]      int32: the heat maps' own "cell" / "pred_cell" fields (rs_maps_field), -1 = none
 *   convs [A]                 host array (device pointers inside), torch layouts: w1 [8][6][3][3], b1 [8], w2 [16][8][3][3], b2 [16]
 *   a2 [A][S][16*P*P]         every agent's flattened trunk output
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL pointer (those inside the first num_agents convs included), num_agents outside
 * 1..RS_MAX_AGENTS, num_samples < 0; a side outside [8, 256] returns RS_ERR_UNSUPPORTED; num_samples == 0 returns RS_OK and launches
 * nothing. */
typedef struct { const float *w1, *b1, *w2, *b2; } rs_cnn_conv_params;
int rs_cnn_sized_team_infer(const float* maps, const int32_t* cells, const int32_t* pcells, int32_t num_agents, int64_t num_samples,
                            int32_t map_side, const rs_cnn_conv_params* convs, float* a2, rs_stream_t stream);

/* rs_cnn_sized_team_eval_head: rs_cnn_team_eval_head with the first layer's depth as an argument, Linear(flat, 32) with flat = 16 p p for
 * an integer p in 4..128: grid = (64-image tiles, agent), four waves on a quarter of k each, exact f32 matrix cores, the four partial
 * sums added in wave order, then the bias (no atomics; an image's bits depend on neither num_envs nor the grid), then rs_cnn_head's
 * arithmetic (out_dim 8) operation for operation and the evaluation's idle rule.
 *   heads [A]             as rs_cnn_team_eval_head's, w1 [32][flat]
 *   a2 [A][N][flat]       rs_cnn_sized_team_infer's output (N = num_envs)
 *   u [N][A], alive [N], act8 [N][A], act [A][N], logp [A][N], y1_out [A][N][32]   as rs_cnn_team_eval_head's; a caller that walks its
 *                         lanes in chunks passes each chunk's own rows (u, alive, act8 offset by the chunk's first lane)
 * RS_ERR_INVALID_ARG, before anything is launched: flat not 16 p p with p in 4..128, and what rs_cnn_team_eval_head refuses. */
int rs_cnn_sized_team_eval_head(const rs_cnn_head_params* heads, int32_t num_agents, int32_t flat, const float* a2, const float* u,
                                const uint8_t* alive, int8_t* act8, int64_t* act, float* logp, float* y1_out, int32_t num_envs,
                                rs_stream_t stream);

/* ---- The policy round of a RAD-TEAM (CNN) team in TRAINING on 27 x 27 maps (radiation_ppo_amd/ppo_cnn.py: CNNCollector._step_glued):
 * at most three launches whatever the team size and the critic mode -- rs_cnn_team_trunk_infer (the actors), rs_cnn_trunk_infer(agent = -1)
 * for a global critic or rs_cnn_team_critic_trunk_infer for one critic per agent, rs_cnn_team_step_head; a bootstrap round is the critic
 * trunk(s) and the heads.
 *
 * rs_cnn_team_critic_trunk_infer: every critic's trunk (4 input channels) in one launch, grid = (image rounds, critic); the result equals
 * num_critics calls of rs_cnn_trunk_infer(agent = -1) with critic c's prepared weights, bit for bit.
 *   maps [S][4][729]; wscratch [C][rs_cnn_trunk_scratch_floats(4)] (rs_cnn_trunk_prepare(4, ...) per critic); a2 [C][S][2704]
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL pointer, num_critics outside 1..RS_MAX_AGENTS, num_samples < 0; num_samples == 0
 * returns RS_OK and launches nothing. */
int rs_cnn_team_critic_trunk_infer(const float* maps, int32_t num_critics, int64_t num_samples, const float* wscratch, float* a2,
                                   rs_stream_t stream);

/* rs_cnn_team_step_head: every actor's and every critic's head behind the trunks in one launch, grid = (64-image tiles, A + C): rows
 * y < A are the actors, rows y >= A the critics.  Every row runs rs_cnn_team_eval_head's first layer, Linear(2704, 32) on the f32 matrix
 * cores, four k-quarters added in wave order, then the bias (no atomics: an env's bits depend on neither num_envs nor the grid).  Behind
 * it an actor row runs rs_cnn_head's out_dim = 8 arithmetic operation for operation -- its y1, action and log-probability are
 * rs_cnn_team_eval_head's bits -- and a critic row rs_cnn_head's out_dim = 1 arithmetic.
 *   actors [A], critics [C]   host arrays (device pointers inside, passed to the kernel by value: a captured graph holds them), torch
 *                             layouts: w1 [32][2704], b1 [32], w2 [16][32], b2 [16], w3 [8][16] / [1][16], b3 [8] / [1]
 *   num_critics               1: a global critic, its value goes to every agent's row; num_agents: critic c serves agent c
 *   a2_actor [A][N][2704], a2_critic [C][N][2704]   the trunks' outputs (N = num_envs)
 *   u [N][A]                  the uniforms of rs_action_uniforms.  Not NULL = a STEP round: the actor rows write act [A][N], slot 0 of
 *                             logp_val_boot [A][3][N] (the row layout rs_store_rows reads) and act8 [N][A] (the drawn action: no idle
 *                             rule), the critic rows slot 1.  NULL = a BOOTSTRAP round: only the critic rows are launched; they write slot 2
 *                             (actors, a2_actor, act and act8 may be NULL)
 *   mask [N] or NULL          an env with mask[n] == 0 writes nothing; a workgroup whose 64 envs are all masked out returns before its k
 *                             loop.  Required in a bootstrap round
 *   y1_out [A + C][N][32]     or NULL: the first layer's pre-activation output of every row (for tests)
 * RS_ERR_INVALID_ARG, before anything is launched: num_agents outside 1..RS_MAX_AGENTS, num_critics neither 1 nor num_agents,
 * num_envs < 1, NULL critics / a2_critic / logp_val_boot or a NULL pointer inside the first num_critics critics; a step round with NULL
 * actors / a2_actor / act / act8 or a NULL pointer inside the first num_agents actors; a bootstrap round without mask. */
int rs_cnn_team_step_head(const rs_cnn_head_params* actors, int32_t num_agents, const rs_cnn_head_params* critics, int32_t num_critics,
                          const float* a2_actor, const float* a2_critic, const float* u, int64_t* act, float* logp_val_boot, int8_t* act8,
                          const uint8_t* mask, float* y1_out, int32_t num_envs, rs_stream_t stream);

/* ---- The same round for square maps of any side 8 <= map_side <= 256 (walls off: 147 x 147, Linear(85 264, 32) behind the trunk), where
 * the workload is a few hundred envs and a grid of 64-env tiles alone would leave most of the device idle: rs_cnn_sized_team_infer (the
 * actors), rs_cnn_sized_infer(agent = -1) for a global critic or rs_cnn_sized_team_critic_infer for one critic per agent,
 * rs_cnn_sized_team_step_head; a bootstrap round is the critic trunk(s) and the heads.
 *
 * rs_cnn_sized_team_critic_infer: every critic's tiled trunk (4 input channels, no cell planes) in one launch, a persistent grid over the
 * (image, tile, critic) units with rs_cnn_sized_team_infer's empty-window shortcut; the result equals num_critics calls of
 * rs_cnn_sized_infer(agent = -1) with critic c's weights, bit for bit.
 *   maps [S][4][M*M]; convs [C] host array (device pointers inside), torch layouts: w1 [8][4][3][3], b1 [8], w2 [16][8][3][3], b2 [16];
 *   a2 [C][S][16*P*P], P = M / 2
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL pointer (those inside the first num_critics convs included), num_critics outside
 * 1..RS_MAX_AGENTS, num_samples < 0; a side outside [8, 256] returns RS_ERR_UNSUPPORTED; num_samples == 0 returns RS_OK and launches
 * nothing. */
int rs_cnn_sized_team_critic_infer(const float* maps, int32_t num_critics, int64_t num_samples, int32_t map_side,
                                   const rs_cnn_conv_params* convs, float* a2, rs_stream_t stream);

/* rs_cnn_sized_team_step_head: rs_cnn_team_step_head at the depth flat = 16 p p (p in 4..128), in two launches.
 * Stage 1, grid = (64-env tiles, k slices, rows): Linear(flat, 32) split over k.  A slice is rs_cnn_sized_team_head_slice_floats()
 * floats (a compile-time constant, a multiple of 128; the last slice is shorter, a multiple of 16), S = ceil(flat / slice) slices: S
 * depends on flat alone.  Within a workgroup four waves take a quarter of the slice each on the f32 matrix cores (exact f32) and their
 * partial sums are added in wave order; the 64 x 32 sums go to scratch [rows][S][N][32].
 * Stage 2, grid = (64-env tiles, rows), one env per lane: the S partial sums in slice order, then the bias, then rs_cnn_head's arithmetic
 * operation for operation (out_dim 8 with the inverse-CDF draw and no idle rule on an actor row, out_dim 1 on a critic row).  No atomics:
 * an env's bits depend on neither num_envs nor the grid.
 *   actors, critics, num_critics, u, act, logp_val_boot, act8, mask, y1_out   as rs_cnn_team_step_head's, w1 [32][flat]; a step round
 *                             (u not NULL) launches the A + C rows, a bootstrap round (u NULL, mask required) the C critic rows, which
 *                             write slot 2
 *   a2_actor [A][N][flat], a2_critic [C][N][flat]   the trunks' outputs (N = num_envs)
 *   scratch, scratch_floats   at least rs_cnn_sized_team_head_scratch_floats(flat, rows launched, num_envs) floats; its contents before the
 *                             call do not matter and it holds nothing of use after it.  A masked-out env writes nothing and reads no
 *                             scratch; a workgroup of stage 1 whose 64 envs are all masked out returns before its k loop
 * rs_cnn_sized_team_head_scratch_floats: num_rows x S x num_envs x 32, or 0 for a flat that is not 16 p p with p in 4..128 (or num_rows
 * or num_envs < 1).
 * RS_ERR_INVALID_ARG, before anything is launched: what rs_cnn_team_step_head refuses, such a flat, a NULL scratch, scratch_floats below
 * the size function's value. */
int32_t rs_cnn_sized_team_head_slice_floats(void);
int64_t rs_cnn_sized_team_head_scratch_floats(int32_t flat, int32_t num_rows, int32_t num_envs); /* 0 for a bad flat */
int rs_cnn_sized_team_step_head(const rs_cnn_head_params* actors, int32_t num_agents, const rs_cnn_head_params* critics,
                                int32_t num_critics, int32_t flat, const float* a2_actor, const float* a2_critic, const float* u,
                                int64_t* act, float* logp_val_boot, int8_t* act8, const uint8_t* mask, float* y1_out,
                                float* scratch, int64_t scratch_floats, int32_t num_envs, rs_stream_t stream);

/* ---- The bootstrap particle filter and the RID-FIM controller on top of it ('rid-fim' in algos/test_environment/eval/test_policy.py:
 * 184-231, 573-574; ParticleFilter, FIC and ssp in eval/core.py:528-620, 655-764, 767-799; radiation_ppo_amd/bpf.py,
 * radiation_ppo_amd/evaluate.py: run_test_environments_rid_fim; csrc/rs_bpf.hpp, csrc/rs_bpf.hip).  Declared ahead of the look-ahead
 * entries, which stay the header's last two.  Everything is float64.
 *
 * Every (env, agent) pair = n * A + a runs a filter of its own over (intensity, x, y); nothing is shared between agents.  The state is
 * the caller's, in device memory (handed over with rs_bpf_state_create):
 *   xp [pairs][3][NP]     particles: intensity in the filter's units (x 1e4 in the measurement model), then x and y in cm
 *   w, logw [pairs][NP]   normalised weights and their logarithms (-inf where w is 0, as np.log gives)
 *   est [pairs][3]        xpHatMean (core.py:613-615); neff [pairs] the effective particle count of the last track
 *   rdiv [pairs]          the controller's latch RDIV_FLAG (core.py:674, 758-759); rs_bpf_track with first != 0 sets it to 1
 *   flags [pairs]         RS_BPF_RESAMPLED: the last track resampled; RS_BPF_ERR_SSP (sticky): the resampler's child counts did not
 *                         add up to NP -- ssp's ValueError (core.py:796-798) --, the particles were left ungathered
 *   scratch               rs_bpf_scratch_bytes(pairs, NP) bytes: a second particle buffer for the gather (the controller keeps each
 *                         move's rates there) and the resampler's child counts.  The resampler's xi are computed where they are read. */
#define RS_BPF_RESAMPLED 1
#define RS_BPF_ERR_SSP 2
#define RS_BPF_MAX_WINDOW 1024     /* interval[0] + interval[1] at most */

/* Both objects are opaque host objects the library makes from the caller's values and pointers (the binding's record of the header's
 * structs with fields is closed); the device memory behind a state stays the caller's.
 * rs_bpf_params_create: the filter's and the controller's settings, in this order:
 *   num_particles           NP >= 2, any (not only multiples of 64)
 *   sigma_xy, sigma_I       proSigma = [noise_params[1], noise_params[0], noise_params[0]] (core.py:540): sigma_I = noise_params[1]
 *   thresh                  resample where neff < thresh * NP (core.py:544, 573)
 *   intensity[2], coord[2]  the uniform prior's box (core.py:556-557); host arrays, copied
 *   alpha, fim_thresh       the Renyi order (not 1) and the latch's threshold (core.py:673-675)
 *   interval[2]             candidate readings z = clip(x0 - interval[0], 1, inf) .. x0 + interval[1] - 1 (core.py:708); host array, copied
 * RS_ERR_INVALID_ARG: a NULL pointer, NP < 2, a negative sigma or thresh, a prior box with hi < lo, alpha == 1 or nan, interval entries
 * below 0 or their sum above RS_BPF_MAX_WINDOW.
 * rs_bpf_state_create: num_pairs (N * A of the handle the calls are made with) and the device pointers listed above.
 * RS_ERR_INVALID_ARG: a NULL pointer, num_pairs < 1. */
typedef struct rs_bpf_params rs_bpf_params;
typedef struct rs_bpf_state rs_bpf_state;
int rs_bpf_params_create(int32_t num_particles, double sigma_xy, double sigma_I, double thresh, const double* intensity, const double* coord,
                         double alpha, double fim_thresh, const int32_t* interval, rs_bpf_params** out);
void rs_bpf_params_destroy(rs_bpf_params* p);
int rs_bpf_state_create(int32_t num_pairs, double* xp, double* w, double* logw, double* est, double* neff, uint8_t* rdiv, uint32_t* flags,
                        void* scratch, size_t scratch_bytes, rs_bpf_state** out);
void rs_bpf_state_destroy(rs_bpf_state* s);

/* bytes of a state's scratch for num_pairs filters of num_particles; 0 for num_pairs < 1 or num_particles < 2 */
size_t rs_bpf_scratch_bytes(int32_t num_pairs, int32_t num_particles);

/* rs_bpf_track: ParticleFilter.track (core.py:554-591) for every pair of a lane with alive[n] != 0; the state of the others is not touched.
 *   first != 0: the uniform prior xp = lo + (hi - lo) u over intensity x coord x coord, w = 1 / NP, logw = log(1 / NP) (:556-561), rdiv = 1
 *   else the process model (:598-601): x, y += sigma_xy z, intensity = max(intensity + sigma_I z, 0)
 *   then the Poisson log-likelihood (:594-596, 603-607) of the reading k = obs[n][a][0] at the agent's position d (the handle's):
 *     R = square(sqrt(|xp_xy - d|^2)), lam = rint(I 1e4 / R) + bkg (the env's own background rate), logw += xlogy(k, lam) - lgamma(k + 1) - lam
 *   w = exp(logw - max), w /= sum, neff = rint(1 / sum w^2) (:569-571); where neff < thresh NP the reference's SSP resampler (ssp,
 *   :767-799) operation for operation on NP - 1 uniforms, one lane per pair walking the chain, the gather, logw = 0 and the
 *   likelihood and normalisation again (:573-579); then est = sum w xp (:615) and logw = log(w) (:588).
 * Draws: Philox, key (seed, global env id), counter (slot, step index of the NEXT rs_step, episode, 192 + a).  Slot 2 p and 2 p + 1 are
 * particle p's: the prior's three uniforms (words 0-1, 2-3 of the first block, 0-1 of the second), or the process model's three normals
 * by Box-Muller in float64 (intensity and x from the first block's pair, y the cosine branch of the second's); slot 2 NP + k is the
 * resampler's uniform k.  Sums are taken lane by lane, wave by wave in a fixed order, not in numpy's pairwise order.
 *   obs [N][A][11], alive [N]
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL handle, params, state, obs or alive, num_pairs not the handle's N * A,
 * scratch_bytes below rs_bpf_scratch_bytes(num_pairs, NP). */
int rs_bpf_track(rs_handle* h, const rs_bpf_params* p, const rs_bpf_state* s, const float* obs, const uint8_t* alive, int32_t first,
                 rs_stream_t stream);

/* rs_ridfim_eval_step: FIC.optim_action with L = 1 (core.py:703-764) for every pair of a lane with alive[n] != 0, one launch.  For each
 * of the eight moves the candidate position c is rs_peek's (the same lane function; a blocked move: the current position) and
 *   J_fish = sum_p w_p (g0^2 s 1e10 + g1^2 s + g2^2 s),  I4 = I_p 1e4, d = c - xp_xy, den = |d|^2, g0 = 1 / den, g_xy = 2 d I4 / den^2,
 *            s = 1 / (I4 / den + bkg)            -- trace(particle_FIM) with scale = diag(1e10, 1, 1) (:686-694; no rint there)
 *   while rdiv[pair] == 1:  J = renyi_div (:696-701) over the candidate readings z above, x0 = obs[n][a][0], with the filter's rounded
 *            rate lam_p at c:  p_z = sum_p w_p pmf(z; lam_p), p_za = sum_p w_p pmf(z; lam_p)^alpha,
 *            J = 1 / (alpha - 1) sum_z p_z (log p_za - alpha log p_z);   with rdiv[pair] == 0:  J = J_fish.
 * The action is the first index of the largest J (np.argmax); rdiv == 1 and max J > fim_thresh clears the latch (:758-759).
 * A nan J (a particle exactly at a candidate position: lam = inf) is treated as np.argmax and np.max treat it: the first nan index
 * is the action and the latch stays as it is.
 * Two rules the reference leaves to IEEE accidents: a z whose p_z is 0 contributes 0 (the reference computes 0 * (-inf + inf) = nan
 * there); and two moves with the same candidate position give bit-equal J (one code path, one reduction order for every move), so
 * ties from blocked moves go to the lowest index, as the reference's do.
 * pmf is evaluated as exp(xlogy(z, lam) - lgamma(z + 1) - lam) at every 16th reading and carried by pmf(z + 1) = pmf(z) lam / (z + 1),
 * pmf(z + 1)^alpha = pmf(z)^alpha lam^alpha (z + 1)^-alpha in between.  A finished lane gets act8 = 8 and nothing else of it is written.
 *   act8 [N][A]; J, J_fish [N][A][8] or NULL
 * RS_ERR_INVALID_ARG, before anything is launched: what rs_bpf_track refuses, a NULL act8. */
int rs_ridfim_eval_step(rs_handle* h, const rs_bpf_params* p, const rs_bpf_state* s, const float* obs, const uint8_t* alive, int8_t* act8,
                        double* J, double* J_fish, rs_stream_t stream);

/* rs_bpf_draws (for tests and the composed runner): the draws rs_bpf_track would consume at the env's present step, through the same
 * device functions, for every pair:  prior_u [N][A][3][NP] uniforms in [0, 1), normals [N][A][3][NP] standard normals (intensity, x, y),
 * resample_u [N][A][NP - 1]; any of the three may be NULL.
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL handle, num_particles < 2. */
int rs_bpf_draws(rs_handle* h, int32_t num_particles, double* prior_u, double* normals, double* resample_u, rs_stream_t stream);

/* rs_bpf_fim: the particles' 3 x 3 Fisher information matrix, FIC.particle_FIM (core.py:686-694; the same expression in
 * test_policy.py:119-126, 146-153, 204-211), for every pair of a lane with alive[n] != 0, one launch, one workgroup per pair:
 *   F[i][j] = sum_p w_p ((g_i g_j) s) c_j          with I4, d, den, g = (g0, g_x, g_y) and s as in rs_ridfim_eval_step above,
 * evaluated at pos[n][a] (NULL: the agent's present position, the handle's) with the env's own background rate.  c is the column
 * scale of J @ scale, so F is not symmetric.
 *   prior == 0: the state's particles and weights, c = (1e10, 1, 1).  trace(F) is J_fish of rs_ridfim_eval_step at that position.
 *   prior != 0: the initial bound (test_policy.py:127-135 with uni_probs of :363-365): the prior's particles, regenerated from the
 *     draws rs_bpf_track(first = 1) consumes at the env's present step (the same device function; nothing is read from xp or w),
 *     weights 1 / NP, c = (1e10 / (I_hi - I_lo), 1 / (c_hi - c_lo), 1 / (c_hi - c_lo)) from the params' prior box.
 * Sums are taken lane by lane, wave by wave in rs_bpf_track's fixed order.  A particle exactly at the position gives inf / nan entries,
 * as numpy does.  None of a finished lane's outputs is written.
 * One difference from the reference, on purpose: its `FIM` and 'rid-fim' `init_est` branches index a 2-vector detector position with
 * [1:], which broadcasts y over both axes (test_policy.py:121, 197, 206); here the position is the detector's (x, y), as the `act`
 * branches and 'bpf-a2c''s `init_est` have it.
 *   alive [N]; pos [N][A][2] or NULL; F [N][A][3][3]; trace [N][A] or NULL: F[0][0] + F[1][1] + F[2][2]
 * RS_ERR_INVALID_ARG, before anything is launched: what rs_bpf_track refuses (its obs aside), a NULL F. */
int rs_bpf_fim(rs_handle* h, const rs_bpf_params* p, const rs_bpf_state* s, const uint8_t* alive, const double* pos, int32_t prior, double* F,
               double* trace, rs_stream_t stream);

/* rs_bpf_a2c_eval_step: the policy round of 'bpf-a2c' (test_policy.py:136-154) -- the trained recurrent actor fed the particle filter's
 * location estimate in place of the PFGRU's -- for every agent of every lane in one launch (csrc/rs_rnn_policy.hip; the grid and the
 * weights of rs_rnn_team_eval_step, default widths only: GRU 24, heads 32 / 32).  On a lane with alive[n] != 0, in order:
 *   x = obs[n][a][0..10] with x[0] = clip((float)(((double)obs0 - mean) / std), -8, 8)     rs_welford_standardize's expression, then
 *                                                                                          the clip of test_policy.py:400, 422
 *   loc = (float)(est[n][a][1..2] / area_max)         est: the filter state's xpHatMean; area_max: the env's search_area[2][1] (:141, 392)
 *   rs_rnn_team_eval_step's arithmetic, operation by operation: GRU, policy head, the draw #{j < 7 : cdf_j <= u}; h updated in place
 *   sim_pos[n][a] = (double)position + ACTION[act]    the controller's own table (:18-27: +-100 and +-71), not the env's step, and no
 *                                                     blocking test (sim_step, :241); position: the handle's
 * A finished lane gets act8 = 8 and nothing else of it is written; a wave without a live lane leaves at once.
 *   weights [num_agents] pointers to RS_RNN_POLICY_WEIGHT_FLOATS floats; obs [N][A][11]; mean, std [N][A]; est [N][A][3];
 *   hid [A][N][24]; u [N][A]; alive [N]; act8 [N][A]; sim_pos [N][A][2]; x_out [N][A][11] and loc_out [N][A][2] or NULL (for tests
 *   and the composed runner)
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL handle or required pointer, a NULL entry among the first num_agents weights,
 * num_agents outside 1..RS_MAX_AGENTS or not the handle's. */
int rs_bpf_a2c_eval_step(rs_handle* h, const float* const* weights, int32_t num_agents, const float* obs, const double* mean, const double* std,
                         const double* est, double area_max, float* hid, const float* u, const uint8_t* alive, int8_t* act8, double* sim_pos,
                         float* x_out, float* loc_out, rs_stream_t stream);

/* ---- The env's look-ahead and the gradient-search baseline on top of it (radiation_ppo_amd/evaluate.py:
 * run_test_environments_gradient_search; csrc/rs_lookahead.hpp, csrc/rs_lookahead.hip).
 *
 * rs_peek: RadSearch.FIM_step (rad_search_env.py:1768-1799) for every agent of every env and all eight moves in one launch, one lane
 * per (env, agent, move), with the measurement a step to the candidate position would take.  For move k of agent a of env n:
 *   start = from_xy[n][a] where given, else the agent's position; tent = start + get_step(k) (:205-224); blocked = tent outside the bbox
 *   by take_action's own test under enforced boundaries (:917-925) or in_obstruction(tent) (:935-937); no collision rule -- FIM_step
 *   passes proposed_coordinates = [] (:1789), the rule of rs_step's single-int form 16 + a; xy = blocked ? start : tent, moved = !blocked.
 *   lam is the rate at xy computed fresh as agent_step computes it for an agent that has moved (:486-512): shortest path, Euclidean
 *   distance r, is_intersect; bkg if intersected, else I / r + bkg (I / r^2 + bkg under falloff 1); r == 0 is taken as 1 and no error
 *   bit is set.  meas = Poisson(lam) from the env's serial sampler: key (seed, global env id), counter (candidate index, step index of
 *   the NEXT rs_step, episode, 128 + 8 a + k) -- streams 128..191, the step and episode words rs_action_uniforms uses.  lam and meas
 *   are computed for an unmoved candidate too (at its start); the gradient search ignores them.
 * NOTHING in the env changes: positions, out-of-bounds counts, flags, distances, error bits, step and episode counters and the output
 * rows are as before, and an rs_step after a peek returns the same bits as one without it.  (The reference's take_action bumps
 * out_of_bounds_count and sets the blocking flag even in a look-ahead.)
 *   from_xy [N][A][2] or NULL; xy [N][A][8][2]; moved [N][A][8]; lam [N][A][8] or NULL; meas [N][A][8] or NULL
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL handle, xy or moved. */
int rs_peek(rs_handle* h, const int32_t* from_xy, int32_t* xy, uint8_t* moved, double* lam, int64_t* meas, rs_stream_t stream);

/* rs_gs_eval_step: the policy round of the gradient-search controller (GradSearch.step, algos/test_environment/eval/core.py:636-653;
 * 'gs' in eval/test_policy.py:73-108) for every agent of every lane in one launch: rs_peek's look-ahead, bit for bit (both kernels run
 * one lane function), then on a lane whose episode runs
 *   g_k = moved_k ? (float)(((double)meas_k - (double)obs[n][a][0]) * 0.01 * q_rec) : 0.0f      (core.py:641-644; q_rec = 1 / q, :624)
 * -- float64 arithmetic rounded once, what assigning a Python float into the reference's float32 `grad` tensor does -- and the action
 * Categorical(softmax(g)).sample() (:649-653) as the inverse-CDF draw of the policy kernels (rs_action.hpp) from u[n][a].  A finished
 * lane (alive[n] == 0) looks nowhere and gets act8 = 8 (idle) and a gradient row of zeros.
 * One difference from the reference: it decides "the move did not take place" by comparing observation coordinates (:641); this uses
 * `moved`.  The two agree except under coord_noise, where the reference compares noisy coordinates and the test means nothing.
 * One evaluation lock-step is rs_action_uniforms, rs_gs_eval_step, rs_step, rs_eval_post_step (its four Welford pointers NULL) on one
 * stream.
 *   obs [N][A][11]        the current observation (element 0: the reading at the agent's position)
 *   u [N][A], alive [N]   the uniforms of rs_action_uniforms; alive[n] != 0 while lane n's episode runs
 *   act8 [N][A]           rs_step's action rows
 *   grad_out [N][A][8]    or NULL: the gradients (for tests)
 * RS_ERR_INVALID_ARG, before anything is launched: a NULL handle, obs, u, alive or act8. */
int rs_gs_eval_step(rs_handle* h, const float* obs, double q_rec, const float* u, const uint8_t* alive, int8_t* act8, float* grad_out,
                    rs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADSEARCH_H */
