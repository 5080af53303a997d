/*
 * crl.h -- C ABI of the MI355X-native vector-env backend (libcrl_hip.so).
 *
 * The reference (ucla-rlcourse/competitive-rl) is pure Python and has NO FFI:
 * its boundary for this path is the Python VecEnv protocol.  Each entry point
 * below names the reference interface it stands in for (file:line relative to
 * /root/reference/competitive_rl/).  The Python host mirror of that protocol
 * (competitive_rl_amd/vec_env.py) is the only in-tree caller; INTEGRATION.md
 * shows the ctypes stub a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative CRL_E* code (crl_last_error() has the text); all
 * device work is ordered on the caller's HIP stream (`stream` is a
 * hipStream_t passed as void*: whatever the caller enqueues there afterwards
 * sees the results; a CarRacing step forks to the context's own streams and
 * joins them back before it returns); a context is bound to one GPU and is not
 * thread-safe; `*_dev` pointers are device memory owned by the caller
 * (e.g. torch tensors), `*_host` pointers are host memory.
 */
#ifndef CRL_H_
#define CRL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- geometry of cPongDouble-v0 (pong/base_pong_env.py:158-211) */
#define CRL_PONG_W 160
#define CRL_PONG_H 210
#define CRL_PONG_TOP 34          /* arena top == top_border_thickness          */
#define CRL_PONG_BOTTOM 194      /* arena bottom = 34 + window_width (sic)     */
#define CRL_PONG_BALL 4
#define CRL_PONG_BAT_W 5
#define CRL_PONG_BAT_H 15
#define CRL_PONG_BATL_X 16
#define CRL_PONG_BATR_X 139
#define CRL_PONG_MIRROR_ROW 25   /* base_pong_env.py:153-154: rows >= 25 flip  */
#define CRL_PONG_MAX_ROUNDS 21   /* pong/register.py:20-22                     */
#define CRL_PONG_MAX_STEPS 10000 /* base_pong_env.py:171                       */
#define CRL_PONG_CHEAT 999       /* base_pong_env.py:9                         */
#define CRL_PONG_FRAME_BYTES (CRL_PONG_H * CRL_PONG_W * 3) /* 100 800 */
/* score band: 22 x 22 (score_l, score_r) images of rows 0..33, gray u8        */
#define CRL_PONG_ATLAS_SCORES 22
#define CRL_PONG_ATLAS_BYTES (22 * 22 * CRL_PONG_TOP * CRL_PONG_W)

enum { CRL_OK = 0, CRL_EINVAL = -1, CRL_EHIP = -2, CRL_ENOMEM = -3, CRL_ESTATE = -4,
       /* an earlier crl_step was given a Pong action outside {0, 1, 2, 999}: the reference asserts
          action_space.contains(action) (pong/base_pong_env.py:42).  Device-resident actions are
          checked by the step kernel; the flag reaches the host without a sync, so the error is
          reported ONCE, by the first crl_step / crl_reset / crl_check that sees it (that call does no
          work; the offending bat did not move), and cleared: the next call proceeds. */
       CRL_EACTION = -5 };

enum crl_env_kind {
    CRL_ENV_PONG_DOUBLE = 1, /* cPongDouble-v0                                                    */
    CRL_ENV_CAR_DOUBLE = 2,  /* cCarRacingDouble-v0                                               */
    /* cPong-v0 (PongSinglePlayerEnv, pong/base_pong_env.py:16-82): the right bat is the AutoBat
       (:445-454) = action 999 on that side; actions int32 (N), one view, obs (N,1,...) raw or
       (N,K,R,R) wrapped, rewards f32 (N) = the left player's */
    CRL_ENV_PONG_SINGLE = 3,
    /* cCarRacing-v0: CarRacing(num_player=1) (car_racing/register.py:11-17, 29-40): one car,
       actions f32 (N,1,2), obs (N,K,96,96), rewards f32 (N,1) */
    CRL_ENV_CAR_SINGLE = 4,
};
/* crl_opts.flags */
#define CRL_FLAG_CAR_NO_CONTACTS 2  /* cCarRacingDouble: skip the car-car contact constraints (cars pass
                                      through each other); default is to solve them */
#define CRL_FLAG_CAR_FMA 4          /* cCarRacing*: b2World.Step's island solver (car_racing_multi_players.py:600 -> b2Island::Solve:
                                      integrators, the 180 velocity and <= 60 position iterations of joints and contacts)
                                      evaluates every a*b+c in ONE fused multiply-add instead of Box2D's two roundings:
                                      0.46 x the instructions of the step's longest dependent chain.  Checked at tolerance 0
                                      against the CPU checker's -DCRL_FMA build (the same sites as MAD / NMAD); one step away from the
                                      checker's libm build by <= 2.7e-5 relative on velocities (default: 5.6e-6),
                                      which is why it is opt-in */
#define CRL_FLAG_STACK_REPLICATE 1 /* FrameStack wrapper semantics (utils/atari_wrappers.py:243-247):
                                      reset fills all K planes with the first frame, instead of
                                      FrameStackTensor's zeroed history */

/* ---- cCarRacingDouble-v0 (car_racing/car_racing_multi_players.py:54-88) */
#define CRL_CAR_MAX_TILES 512 /* tiles of one track (reference tracks: 230-380) */
#define CRL_CAR_OBS 96        /* STATE_W = STATE_H = 96 */
/* The pre-rastered observation map (render_road_for_observation_map, car_racing_multi_players.py:732-755):
   the reference draws into a 10000 x 10000 surface; everything that is not grass lies inside the window
   [CRL_CAR_MAP_ORG, CRL_CAR_MAP_ORG + CRL_CAR_MAP_W)^2 of it (1.7636 px per world unit, origin at 5000),
   which is what a context keeps per env: 7-colour palette, 4 bits per pixel, 739 328 bytes. */
#define CRL_CAR_MAP_ORG 4392
#define CRL_CAR_MAP_W 1216
/* reward read-out of the indicator strip: bitmaps of "%05.0f" % r for r = -999..2000 plus "-0000",
   10 rows of 32 bits each (competitive_rl_amd/assets/car_reward_text.npz) */
#define CRL_CAR_TEXT_STRINGS 3001
#define CRL_CAR_TEXT_ROWS 10
#define CRL_CAR_TEXT_RMIN (-999)

enum crl_obs_mode {
    /* raw env: obs (N,2,210,160,3) u8, 1 step = 1 frame
       (PongDoublePlayerEnv._step, pong/base_pong_env.py:113-142) */
    CRL_OBS_RAW_RGB = 0,
    /* make_env_a2c_atari stack: skip-4 + max-2 + gray + INTER_AREA resize
       (utils/atari_wrappers.py:40-53,89-219), obs (N,2,K,R,R) u8 with
       FrameStackTensor roll/zero-on-done semantics for K>1 (utils/utils.py:145-173) */
    CRL_OBS_GRAY_RESIZED = 1,
};

/* One raster-ready frame of the game, 8 bytes (what Arena/Ball/Bat/Scoreboard.draw
 * read: base_pong_env.py:259-266).  ball_x/ball_y are int16 because a bat hit can
 * place the ball a few px outside the arena rows (it is clipped when drawn). */
typedef struct crl_pong_frame {
    int16_t ball_x, ball_y;
    uint8_t bat_l_y, bat_r_y;
    uint8_t score_l, score_r; /* score_l == 255 marks a BLANK (all-zero) plane */
} crl_pong_frame;

/* Per-env state exchanged by crl_get_state / crl_set_state (host side, AoS).
 * On the device the same fields live in SoA arrays (DESIGN.md "HBM layout"). */
typedef struct crl_pong_env_state {
    double speed_x, speed_y;       /* Ball._speed_x/_speed_y (f64)                  */
    int32_t ball_x, ball_y;        /* Ball._rect.x/.y                               */
    int32_t bat_l_y, bat_r_y;      /* Bat._rect.y                                   */
    int32_t score_l, score_r;      /* PongGame._score_left/_right                   */
    int32_t num_rounds, num_steps; /* PongGame._num_rounds/_num_steps               */
    uint32_t serve_ctr;            /* serves drawn so far (RNG / replay cursor)     */
    int32_t wrap_steps;            /* ClipRewardEnv._steps (atari_wrappers.py:169)  */
    crl_pong_frame keep[2];        /* MaxAndSkipEnv._obs_buffer as frames (:104-116)*/
    crl_pong_frame hist[3][2];     /* frame_stack>1: the 3 older planes of the stack,
                                      oldest first, each the (keep0, keep1) pair that
                                      produced it; BLANK = plane zeroed by a done
                                      (FrameStackTensor.update, utils/utils.py:158-170) */
} crl_pong_env_state;              /* 120 bytes */

typedef struct crl_opts {
    int32_t env_kind;    /* crl_env_kind                                             */
    int32_t obs_mode;    /* crl_obs_mode                                             */
    int32_t resized_dim; /* Pong: R = 84 or 42 (make_envs.py:67 resized_dim), 0 for raw;
                            CarRacing: ignored                                       */
    int32_t frame_stack; /* K planes per agent in GRAY_RESIZED mode (1 or 4)         */
    int64_t num_envs;    /* envs owned by THIS context (one shard)                   */
    int64_t env_id_base; /* global id of env 0 of this shard: RNG is keyed by global
                            id so results do not depend on how envs are sharded      */
    uint64_t seed;       /* make_envs(seed=...)                                      */
    int32_t device;      /* HIP device ordinal                                       */
    int32_t flags;       /* CRL_FLAG_*                                                  */
    int32_t action_repeat; /* CarRacing(action_repeat=...) (car_racing_multi_players.py:162,576):
                              0 or 1 = none, at most 16; Pong: must be 0                */
    int32_t done_policy;   /* CarRacing: crl_car_done_policy; Pong: must be 0           */
    int32_t obs_dtype;     /* crl_obs_dtype of obs_dev (GRAY_RESIZED Pong contexts; others: U8) */
    int32_t reserved;      /* must be 0                                                 */
} crl_opts;

/* Which cars end an env's episode under the VecEnv (CarRacing contexts) */
enum crl_car_done_policy {
    /* make_car_racing_double: FlattenMultiAgentObservation returns any(done.values())
       (utils/atari_wrappers.py:329-330) */
    CRL_CAR_DONE_ANY = 0,
    /* make_competitive_car_racing: CarRacingWrapper returns d[0]
       (car_racing/make_competitive_car_racing.py:24-33); a finished car 1 stays in the world,
       frozen (car_racing_multi_players.py:578-579), while car 0 drives on */
    CRL_CAR_DONE_CAR0 = 1,
};
/* Element type of the observation tensor handed to crl_reset / crl_step / crl_render */
enum crl_obs_dtype {
    CRL_OBS_U8 = 0,
    /* DummyVecEnv's observation buffers are float32 holding 0..255 (utils/dummy_vec_env.py:37-44;
       SURVEY 8d config-3 variant, 225 792 B/env): same values, widened in the raster's store */
    CRL_OBS_F32 = 1,
    /* The reference's own float32 values.  Old gym's Box defaults to float32, so MaxAndSkipEnv's buffers are float32
       (utils/atari_wrappers.py:104-116) and WarpFrame.parse_single_frame (:215-219) runs cv2.cvtColor / cv2.resize on FLOAT
       frames during step(): the observation is the UNROUNDED INTER_AREA average of gray = R*0.299f + G*0.587f + B*0.114f
       (e.g. 254.99998 where the uint8 path says 255); reset() -- and the auto-reset of a finished env -- goes through the
       uint8 image and yields rounded values.  A plane whose two kept frames are the same frame is such a reset observation.
       A per-score-pair table of the court without ball and bats + an exact re-draw of the ~150 pixels around them, patched into the pieces
       before they are stored: 2.8 ms per step at 65 536 envs x (2, 4, 84, 84) (23.5 M env-steps/s), HBM traffic 1.005 x the tensor;
       CRL_OBS_F32 (the uint8 values, widened) takes 2.6 ms. */
    CRL_OBS_F32_REF = 2,
};

typedef struct crl_ctx crl_ctx;

/* make_envs(...) -> VecEnv construction (make_envs.py:67-118; DummyVecEnv.__init__
 * dummy_vec_env.py:26-46).  `score_atlas_host`: CRL_PONG_ATLAS_BYTES gray values of
 * the top band for every score pair (Scoreboard.draw, base_pong_env.py:474-487).  CarRacing
 * contexts take the reward-text bitmaps instead (uint32 [CRL_CAR_TEXT_STRINGS][CRL_CAR_TEXT_ROWS],
 * draw_text, car_racing/pygame_rendering.py:16-18) or NULL to leave the text out. */
int crl_create(const crl_opts *opts, const uint8_t *score_atlas_host, crl_ctx **out);

/* VecEnv.close (dummy_vec_env.py:77-79; idempotent like subproc_vec_env.py:131-141) */
void crl_destroy(crl_ctx *ctx);

/* VecEnv.seed(seed): env i gets seed + i (dummy_vec_env.py:65-69).  In the reference
 * this never reaches Pong's RNG (_seed is a no-op, base_pong_env.py:38-39); here it
 * re-keys the counter-based serve sampler. */
int crl_seed(crl_ctx *ctx, uint64_t seed);

/* VecEnv.reset() (dummy_vec_env.py:71-75): resets every env, writes the first
 * observation into obs_dev (layout per obs_mode). */
int crl_reset(crl_ctx *ctx, uint8_t *obs_dev, void *stream);

/* VecEnv.step(actions) = step_async + step_wait (base_vec_env.py:178-187,
 * dummy_vec_env.py:48-63) with auto-reset.  actions_dev: Pong int32 (N,2), each 0/1/2 or
 * 999; CarRacing float32 (N,2,2) = per car (steer, gas-or-brake) in [-1,1]; CarRacing obs is
 * (N,2,96,96) u8, rew (N,2) per-car step rewards, done (N) = any car done or TimeLimit.  obs_dev: per obs_mode.  rew_dev: f32 (N,2) (raw: game reward; wrapped:
 * np.sign of the 4-frame sum).  done_dev: u8 (N).  Any output pointer may be NULL
 * to skip that output (obs_dev NULL = dynamics only). */
int crl_step(crl_ctx *ctx, const void *actions_dev, uint8_t *obs_dev, float *rew_dev,
             uint8_t *done_dev, void *stream);

/* ---- step_envs' observation stack fused into the step (utils/utils.py:23-60 calls FrameStackTensor.update :158-170 on the
 * learner's observation with mask = 1 - done right after envs.step).  A GRAY_RESIZED Pong context keeps the descriptors of every
 * env's last four planes with exactly that history rule (planes of an episode that ended are erased, the first observation of the
 * next one is the newest plane), so the stack the trainer would roll and append -- 13.4 GB of traffic per step for 65 536 x
 * (4, 84, 84) float32 -- is DRAWN by the launch that draws the observation: written once, never read.
 *   stack_dev     (N, planes, R, R) of agent `agent`, planes oldest to newest, u8 or f32 per `dtype` (CRL_OBS_U8 | CRL_OBS_F32; a
 *                 float32 context -- CRL_OBS_F32 / CRL_OBS_F32_REF -- writes its own float values and needs dtype = CRL_OBS_F32)
 *   valid_planes  updates since the trainer's FrameStackTensor.reset(), capped at `planes`: the older planes are zeros
 *   alias_newest  1: the (agent, newest plane) tile of obs_dev is NOT written -- the caller hands out the stack's newest plane as
 *                 that agent's observation (needs a context with frame_stack = 1 and equal element types)
 * Contexts with CRL_FLAG_STACK_REPLICATE (the FrameStack wrapper's history) and raw contexts refuse (CRL_ESTATE). */
typedef struct crl_stack_desc {
    void *stack_dev;
    int32_t planes;       /* k = 1..4 */
    int32_t dtype;        /* crl_obs_dtype: CRL_OBS_U8 or CRL_OBS_F32 */
    int32_t agent;        /* 0 = the learner (step_envs takes obs[0], utils/utils.py:55-58) */
    int32_t valid_planes;
    int32_t alias_newest;
    int32_t reserved;     /* must be 0 */
} crl_stack_desc;
/* crl_step + the stack: envs.step(actions) followed by frame_stack_tensor.update(obs[0], 1 - done) (utils/utils.py:30,57-58).
 * stack == NULL is crl_step.  obs_dev may be NULL (stack only). */
int crl_step_stack(crl_ctx *ctx, const void *actions_dev, uint8_t *obs_dev, float *rew_dev, uint8_t *done_dev,
                   const crl_stack_desc *stack, void *stream);
/* The stack of the CURRENT state without stepping: frame_stack_tensor.update(envs.reset()) of the training scripts, and what the
 * host mirror compares a trainer's own tensor with before it binds it.  obs_dev (optional) is re-drawn as by crl_render. */
int crl_draw_stack(crl_ctx *ctx, uint8_t *obs_dev, const crl_stack_desc *stack, void *stream);

/* The raw observation of the CURRENT state drawn into a buffer that already holds an earlier frame of these envs -- the draw of
 * crl_step / crl_render (VecEnv.step's observation, dummy_vec_env.py:48-63; PongGame.draw + the mirrored second view,
 * pong/base_pong_env.py:259-266, 149-155), storing only what differs.  RAW_RGB Pong contexts (CRL_ESTATE otherwise).
 *   obs_dev      (N, views, 210, 160, 3) u8 as crl_step's, 16-byte aligned
 *   drawn_dev    uint64 (N), 8-byte aligned, the caller's record: the descriptors (crl_pong_frame) obs_dev holds now; written with
 *                the descriptors drawn by this call.  Must not overlap obs_dev.
 *   drawn_valid  0: the record is unknown -- the whole observation is drawn and the record written; otherwise the call stores only the
 *                16-byte chunks whose bytes can differ between the record and the current state (ball and bat rectangles, the score
 *                band when a score changed, the whole frame when exactly one of the two is blank), each with the same bytes the full
 *                draw stores.
 * The caller vouches that nothing has written obs_dev since the call that recorded drawn_dev: a record that does not match the buffer
 * gives a wrong observation.  Timed in slot 1 (crl_kernel_timing) like the draw of crl_step.  Use crl_step_stack with obs_dev NULL
 * to step without drawing. */
int crl_draw_raw_delta(crl_ctx *ctx, uint8_t *obs_dev, uint64_t *drawn_dev, int32_t drawn_valid, void *stream);

/* crl_step with obs_dev NULL followed by crl_draw_raw_delta(obs_dev, drawn_dev, 1), as ONE launch: every env is stepped and the chunks
 * of its observation that differ from the record are stored by the wavefront that stepped it.  Same state, rewards, done flags,
 * record and pixels as the two calls.  RAW_RGB Pong contexts (CRL_ESTATE otherwise); actions_dev, rew_dev and done_dev as crl_step's
 * (the last two optional), obs_dev and drawn_dev as crl_draw_raw_delta's with drawn_valid = 1: the caller vouches that drawn_dev
 * describes obs_dev.  A refused call (an argument, or the report of an earlier out-of-range action) steps nothing and leaves the
 * buffer and the record as they were.  Timed in slot 1 as one launch: slot 0 gets no entry.  With an event set by
 * crl_set_flags_event the call makes the two launches itself, the event between them (slots 0 and 1 as before). */
int crl_step_raw_delta(crl_ctx *ctx, const void *actions_dev, uint8_t *obs_dev, uint64_t *drawn_dev, float *rew_dev, uint8_t *done_dev,
                       void *stream);

/* A hipEvent_t of the caller's (NULL: none) that every crl_step / crl_step_stack records on the step's stream right BEHIND the kernel
 * that writes rew_dev / done_dev and IN FRONT of the observation's draw.  The reference's step_envs walks the done flags on the host
 * after every step (utils/utils.py:33-42); a stream that waits for this event can copy them out while the step's 1-2 ms of raster
 * still run, so the host's books and the next step's launch overlap the draw instead of following it.  Pong contexts.  The event is
 * the caller's: it must belong to the context's device and stay alive until the context is destroyed or the event is unset (NULL). */
int crl_set_flags_event(crl_ctx *ctx, void *event);

/* info[i]["real_reward"], info[i]["num_steps"] (ClipRewardEnv.step,
 * atari_wrappers.py:175-181) as device arrays valid until the next step:
 * real_reward f32 (N,2), num_steps i32 (N). */
int crl_info(crl_ctx *ctx, const float **real_reward_dev, const int32_t **num_steps_dev);
/* Same data copied (device to device, on `stream`) into caller-owned arrays; either
 * destination may be NULL. */
int crl_copy_info(crl_ctx *ctx, float *real_reward_out_dev, int32_t *num_steps_out_dev, void *stream);

/* info[i]["terminal_observation"] (dummy_vec_env.py:55-57), produced lazily: renders,
 * for `count` env indices (host array), the observation the episode ended on at the
 * most recent step where that env was done.  out_dev: raw (count,2,210,160,3) or
 * wrapped (count,2,R,R) u8; CarRacing (count,players,96,96) u8 = the frames drawn just before the
 * auto-reset (with a K-stack the caller prepends the K-1 newest planes it already holds). */
int crl_terminal_observation(crl_ctx *ctx, const int64_t *env_idx_host, int64_t count,
                             uint8_t *out_dev, void *stream);

/* The same with the env indices in DEVICE memory (e.g. torch.nonzero(done)): descriptors are gathered
 * by a kernel and drawn on `stream` -- no device-to-host copy, no allocation (a scratch buffer grows
 * on demand), no synchronisation.  This is what the host mirror's lazy infos use to fetch every
 * finished env of a step in one call. */
int crl_terminal_observation_dev(crl_ctx *ctx, const int64_t *env_idx_dev, int64_t count,
                                 uint8_t *out_dev, void *stream);

/* Synchronises `stream` and reports (then clears) a pending CRL_EACTION. */
int crl_check(crl_ctx *ctx, void *stream);

/* RULE_BASED's action as a label (a teacher's labels for "ppo update, teacher targets").  labels_dev[i * stride], int32, = the action
 * in 0..2 that the cheat code CRL_PONG_CHEAT would resolve to for bat `seat` (0 the left, 1 the right) of env i on the FIRST frame of
 * the next step, in the state the context holds now: auto_action (base_pong_env.py:457-471) + 1, on the ball's speed towards that side
 * (seat 0: -speed_x), the bat's centre bat_y + 7 and the ball's centre ball_y + 2, as the step's decode forms them.  A wrapped step
 * re-evaluates the rule on each of its four frames; the label is the first of them.  One small launch, one lane per env, ordered on
 * `stream` behind the step that committed the state; reads the state and changes nothing in the env.  Refuses (CRL_EINVAL, before
 * any GPU call) a null argument, a CarRacing context, a seat outside {0, 1}, a stride < 1 and a labels_dev that is not 4-byte aligned. */
int crl_rule_labels(crl_ctx *ctx, int32_t seat, int32_t *labels_dev, int64_t stride, void *stream);

/* Parity tests + checkpoint/resume: whole-state copy, host AoS <-> device SoA.
 * Synchronises `stream`. */
int crl_get_state(crl_ctx *ctx, crl_pong_env_state *state_host, int64_t first, int64_t count,
                  void *stream);
int crl_set_state(crl_ctx *ctx, const crl_pong_env_state *state_host, int64_t first,
                  int64_t count, void *stream);

/* Replay mode for the serve sampler: per env a recorded stream of
 * `per_env` draws (u in [0,1), bit_x, bit_y); serve k of env i uses entry
 * [i*per_env + (k % per_env)].  Pass per_env = 0 to return to the Philox sampler. */
int crl_set_replay(crl_ctx *ctx, const double *u_host, const uint8_t *bx_host,
                   const uint8_t *by_host, int64_t per_env);

/* Render arbitrary frames (tests, get_images()/render(), base_vec_env.py:189-217).
 * frames_host: `count` frames; out_dev: (count,2,210,160,3) u8. */
int crl_render_raw(crl_ctx *ctx, const crl_pong_frame *frames_host, int64_t count,
                   uint8_t *out_dev, void *stream);

/* ---- observations by descriptor (BASELINE config #5: every GPU ends up with all N observations)
 * The reference's "gather" is _flatten_obs over the workers' pixel arrays (utils/subproc_vec_env.py:188-222).  Here a frame
 * is a pure function of its 8-byte descriptors, so shards exchange those: crl_obs_descriptors copies the descriptors the
 * current observation was drawn from -- crl_pong_frame [8][N]: stack plane p (0 oldest .. 3 newest), kept frame s (the two
 * frames MaxAndSkipEnv takes the maximum of) in row 2p + s; raw contexts and frame_stack = 1 use rows 6 and 7 -- and
 * crl_render_frames_dev draws `count` observations from descriptors in that layout ([8][count], anyone's), out_dev as
 * crl_step's obs_dev for `count` envs.  64 bytes per env instead of 56 448 (fused 4-stack) or 201 600 (raw). */
int crl_obs_descriptors(crl_ctx *ctx, crl_pong_frame *desc_out_dev, void *stream);
int crl_render_frames_dev(crl_ctx *ctx, const crl_pong_frame *desc_dev, int64_t count, uint8_t *out_dev, void *stream);

/* Re-draws the CURRENT state into obs_dev without stepping (after crl_set_state /
 * crl_car_set_state, or for VecEnv.render): same layout as crl_step's obs_dev. */
int crl_render(crl_ctx *ctx, uint8_t *obs_dev, void *stream);

/* Bytes of one env's observation in the context's obs_mode. */
int64_t crl_obs_bytes_per_env(const crl_ctx *ctx);

/* Launch-level timing hook for bench.py: wraps the `which`-th kernel of crl_step
 * (0 = dynamics, 1 = raster) in hipEvents on the launch stream and accumulates.
 * crl_kernel_time_ms() synchronises and returns total ms and launch count. */
int crl_kernel_timing(crl_ctx *ctx, int enable);
int crl_kernel_time_ms(crl_ctx *ctx, int which, double *total_ms, int64_t *launches);
/* The same with the longest launch, and one more slot for CarRacing contexts: which = 2 is the touching solve (car_touch_kernel, the
 * island solve of the envs whose cars touch: b2World.Step, car_racing_multi_players.py:600), the kernel a steady-state step ends with. */
int crl_kernel_time_stats(crl_ctx *ctx, int which, double *total_ms, int64_t *launches, double *max_ms);

/* ---- cCarRacingDouble state exchange (parity tests, checkpoint) ---------------------- */
typedef struct crl_car_body { /* b2Body: centre of mass, angle, velocities */
    float cx, cy, a, vx, vy, w;
} crl_car_body;

typedef struct crl_car_state {   /* one car: Car (car_dynamics.py:55-129) + its env bookkeeping */
    crl_car_body hull, wheel[4];
    float imp[4][3], motor_imp[4], motor_speed[4]; /* revolute joints hull<->wheel          */
    int32_t limit_state[4];
    double gas[4], omega[4], phase[4];             /* wheel attributes                       */
    double reward, prev_reward;                    /* CarRacing.rewards / prev_rewards       */
    int32_t tile_visited_count, last_block, done, step_count, first_step, pad;
    uint32_t wheel_tiles[4][CRL_CAR_MAX_TILES / 32]; /* w.tiles as bit sets                  */
    uint32_t visited[CRL_CAR_MAX_TILES / 32];        /* tile.road_visited[car]               */
    float sleep_time[5], pad2;                       /* b2Body::m_sleepTime: hull, wheels 0-3 */
} crl_car_state;

#define CRL_CAR_MAX_CONTACTS 8
typedef struct crl_car_contact { /* a touching contact between a fixture of car 0 and one of car 1 */
    int32_t pair;           /* fa * 8 + fb; fixtures 0-3 hull polygons, 4-7 wheels               */
    int32_t count, type;    /* manifold points (1-2); 0 = face of A is the reference, 1 = of B   */
    float ln[2], lp[2];     /* manifold local normal / point (reference body frame)              */
    float pt[2][2];         /* manifold points (incident body frame)                             */
    uint32_t id[2];         /* contact feature ids (warm-start key)                              */
    float nimp[2], timp[2]; /* accumulated normal / tangent impulses                             */
} crl_car_contact;

typedef struct crl_car_env_state {
    crl_car_state car[2];
    int32_t elapsed;  /* gym TimeLimit._elapsed_steps */
    uint32_t episode; /* resets so far                */
    int32_t n_contact;
    int32_t coupled; /* (get only) 1 = the step filed the env for the narrow phase: the cars' boxes met, or the cars touched in the step before */
    crl_car_contact contact[CRL_CAR_MAX_CONTACTS];
} crl_car_env_state;

int crl_car_get_state(crl_ctx *ctx, crl_car_env_state *state_host, int64_t first, int64_t count, void *stream);
int crl_car_set_state(crl_ctx *ctx, const crl_car_env_state *state_host, int64_t first, int64_t count, void *stream);
/* Track of env `env` as the physics keeps it: n tiles; tile_poly float32 [n][5][2] (counter-clockwise, as
 * b2PolygonShape stores them), border_poly float32 [n][4][2], border u8 [n] (0 none, 1 white, 2 red),
 * start_pose = track[0] (beta, x, y). */
int crl_car_get_track(crl_ctx *ctx, int64_t env, int32_t *n, float *tile_poly, float *border_poly, uint8_t *border,
                      float *start_pose, void *stream);
/* Replaces the track of env `env` (parity tests: a track built elsewhere).  The polygons are the reference's
 * road_poly entries in float64 and in its vertex order (_create_track, car_racing_multi_players.py:400-441):
 * tile i = (road1_l, road_m, road1_r, road2_r, road2_l), border quad (b1_l, b1_r, b2_r, b2_l) where border[i] != 0.
 * Derives the float32 sensors and re-rasters the env's observation map (render_road_for_observation_map, :732-755). */
int crl_car_set_track(crl_ctx *ctx, int64_t env, int32_t n, const double *tile_poly, const double *border_poly,
                      const uint8_t *border, const float *start_pose, void *stream);
/* The env's pre-rastered observation map, one palette index per pixel (0 grass, 1 lighter square, 2-4 road
 * 102 / 104 / 107, 5 white, 6 red): palette_host u8 [CRL_CAR_MAP_W][CRL_CAR_MAP_W]; *overflow (optional) = polygon
 * vertices that fell outside the window at the env's last reset (0 for every track). */
int crl_car_get_map(crl_ctx *ctx, int64_t env, uint8_t *palette_host, int32_t *overflow, void *stream);
/* How often a fixed capacity of the device state was hit since crl_create (synchronises `stream`): out4_host[0] = a wheel
 * touching more than 6 track tiles at once (w.tiles is a set in the reference, car_racing_multi_players.py:111-153; the extra
 * tile is not recorded), [1] = more than CRL_CAR_MAX_CONTACTS manifolds between the two cars of an env (the rest are dropped),
 * [2], [3] reserved.  Zero on every track of the tests and of a 10^7 env-step soak: a non-zero count means a deviation. */
int crl_car_cap_hits(crl_ctx *ctx, int32_t *out4_host, void *stream);
/* Car track draws (rules.car_track_draws restates this in numpy; the generator and key of "league draws" below; it does not depend
 * on how a batch is cut into shards).  CarRacing.reset tries _create_track until a lap closes (car_racing_multi_players.py:454-525);
 * attempt a = 0, 1, ... of a reset takes 24 uniforms u[0..23] -- checkpoint c reads u[2c] for its angle's noise and u[2c + 1] for its
 * radius -- and one swap bit for np.random.shuffle of the two birth places.  In a seeded context they are 13 Philox4x32-10 calls:
 *   for k = 0..12:  w = Philox4x32-10(counter = (gid & 0xFFFFFFFF, gid >> 32, (episode << 12 | a << 4 | k) mod 2^32, 0x43415253 "CARS"),
 *                                    key = (seed & 0xFFFFFFFF, seed >> 32)), words w0..w3;
 *   k < 12:   u[2k] = ((w0 << 32 | w1) >> 11) * 2^-53,  u[2k + 1] = ((w2 << 32 | w3) >> 11) * 2^-53: multiples of 2^-53 in [0, 1), exact;
 *   k = 12:   swap = w0 & 1 (w1..w3 unused).  swap = 1: car 0 starts from birth place 1, car 1 from place 0; a one-car context's car
 *             starts from place 0 whatever the bit.
 * gid = env_id_base + i, the env's GLOBAL id; seed = crl_opts.seed or the last crl_seed; episode = the env's count of resets so far
 * (uint32: 0 for the track of the first crl_reset, the `episode` field of crl_car_env_state, which a reset increments); a < 256: a
 * reset whose 256 attempts all fail leaves an empty track.  The track is that of the FIRST attempt that closes a lap, and the swap
 * bit is THAT attempt's, not attempt 0's.  The counter keeps the low 20 bits of the episode: episodes e and e + 2^20 draw the same.
 * Nothing else enters: a track is a function of (seed, gid, episode), whether the reset walks it itself or takes the walk laid
 * ahead beside the steps; crl_seed and crl_car_set_replay void every walk laid ahead under the old key or stream.
 *
 * Replay mode for CarRacing.reset's randomness: per env `attempts` rows of 24 uniforms (the
 * np_random.uniform draws of one _create_track attempt) and one birth-place swap bit each;
 * attempt a of episode `episode` reads row (16 * episode + a) mod attempts of its env.
 * attempts = 0 (null arrays) returns to the Philox draws above. */
int crl_car_set_replay(crl_ctx *ctx, const double *u_host, const uint8_t *swap_host, int64_t attempts);

/* CarRacing.step's per-car returns that the VecEnv folds away, as device arrays valid until the
 * next step: done_car u8 (N, players) = the `done` dict (car_racing_multi_players.py:618),
 * num_steps i32 (N) = info[k]["num_steps"] = CarRacing.step_count after the step (:616-620),
 * captured before the auto-reset. */
int crl_car_info(crl_ctx *ctx, const uint8_t **done_car_dev, const int32_t **num_steps_dev);
/* Same data copied (device to device, on `stream`) into caller-owned arrays, plus elapsed i32 (N) = gym TimeLimit's
 * _elapsed_steps after the step, before the auto-reset (info["TimeLimit.truncated"] is set on the step where it reaches
 * max_episode_steps = 1000, car_racing/register.py:15-26); any destination may be NULL. */
int crl_car_copy_info(crl_ctx *ctx, uint8_t *done_car_out_dev, int32_t *num_steps_out_dev, int32_t *elapsed_out_dev, void *stream);

/* ---- FrameStackTensor.update on device (utils/utils.py:158-170) -----------------
 * stack f32 (N, C*k, H, W), in place:  stack *= mask[n];  planes shift down by C (roll -C on dim 1);
 * the last C planes = obs.  One pass over the tensor (torch's mul + roll + slice-assign are three).
 * obs: (N, C, H, W) with `obs_env_stride` ELEMENTS between envs (a view of a wider tensor is fine),
 * u8 or f32 per `obs_dtype` (crl_obs_dtype); mask: f32 (N) or NULL (= all ones).  hw = H*W. */
int crl_frame_stack_update(float *stack_dev, const void *obs_dev, int32_t obs_dtype, int64_t obs_env_stride,
                           const float *mask_dev, int64_t n, int32_t c, int32_t k, int64_t hw, void *stream);
/* The same update OUT of place: dst = (src * mask) shifted, with obs as the newest planes; src is not written.  This is the
 * reference's own data flow -- `self.current_obs = self.current_obs.roll(...)` (utils/utils.py:166-167) binds a NEW tensor on every
 * update -- and a plain streaming copy for the memory system (no load that must stay ahead of a store to the same rows).  dst and
 * src must not overlap (CRL_EINVAL). */
int crl_frame_stack_update_to(float *dst_stack_dev, const float *src_stack_dev, const void *obs_dev, int32_t obs_dtype, int64_t obs_env_stride,
                              const float *mask_dev, int64_t n, int32_t c, int32_t k, int64_t hw, void *stream);
/* The same update of a UINT8 stack (N, C*k, H, W) -- `FrameStackTensor(..., dtype=torch.uint8)`, an opt-in beside the reference's float32
 * contract (utils/utils.py:145-157 allocates float32) --, in place (dst == src) or into another tensor (no overlap: CRL_EINVAL).  Bytes
 * cannot be scaled: a mask entry of 0 erases the env's history, any other value keeps it (the masks of step_envs are 1 - done,
 * utils/utils.py:55-57); a float32 observation holds 0..255 integers and is truncated as a tensor cast would. */
int crl_frame_stack_update_u8(uint8_t *dst_stack_dev, const uint8_t *src_stack_dev, const void *obs_dev, int32_t obs_dtype, int64_t obs_env_stride,
                              const float *mask_dev, int64_t n, int32_t c, int32_t k, int64_t hw, void *stream);

/* ---- built-in CNN opponents of cPongTournament-v0 ----------------------------
 * Stands in for utils/policy_serving.py:10-66 `Policy(..., use_light_model=True)` as built by
 * pong/builtin_policies.py:61-91 for WEAK / MEDIUM: LightActorCritic (utils/network.py:73-93:
 * x/255 -> conv 4->16 k4 s2 -> ReLU -> conv 16->16 k2 s2 -> ReLU -> 1600 -> 3 logits) on the
 * policy's OWN stack of the last four 42x42 frames it was shown (FrameStackTensor.update without
 * a mask, utils/utils.py:159-170: never cleared at episode ends), action = argmax of the logits.
 * Weights are the model tensors of the checkpoint, float32, in torch layout. */
#define CRL_POLICY_DIM 42
#define CRL_POLICY_STACK 4
typedef struct crl_policy crl_policy;
int crl_policy_create(int32_t device, int64_t num_envs, const float *conv1_w_host /*[16,4,4,4]*/,
                      const float *conv1_b_host /*[16]*/, const float *conv2_w_host /*[16,16,2,2]*/,
                      const float *conv2_b_host /*[16]*/, const float *actor_w_host /*[3,1600]*/,
                      const float *actor_b_host /*[3]*/, crl_policy **out);
/* Policy(..., use_light_model=False) (policy_serving.py:21-25): ActorCritic (utils/network.py:14-50: conv 4->16 k4 s2, conv 16->32 k4
 * s2 pad 2, conv 32->256 k11, actor 256->3) -- the model of the reference's STRONG / ALPHA_PONG opponents -- behind the same
 * handle: crl_policy_reset / _act / _get_stack / _set_stack / _destroy work on it unchanged. */
int crl_policy_create_full(int32_t device, int64_t num_envs, const float *conv1_w_host /*[16,4,4,4]*/,
                           const float *conv1_b_host /*[16]*/, const float *conv2_w_host /*[32,16,4,4]*/,
                           const float *conv2_b_host /*[32]*/, const float *conv3_w_host /*[256,32,11,11]*/,
                           const float *conv3_b_host /*[256]*/, const float *actor_w_host /*[3,256]*/,
                           const float *actor_b_host /*[3]*/, crl_policy **out);
void crl_policy_destroy(crl_policy *p);
/* Policy.reset (policy_serving.py:46-47): zero the frame stack. */
int crl_policy_reset(crl_policy *p, void *stream);
/* Policy.__call__ (policy_serving.py:58-66): push one 42x42 u8 frame per env (env i at
 * frame_dev + i * frame_stride bytes; stride a multiple of 4) onto the stack and write the
 * greedy action of env i to actions_dev[i * action_stride] (int32 elements; pass 2 to fill the
 * right-hand column of an (N, 2) cPongDouble action array in place).  logits_dev: optional
 * float32 [N, 3]. */
int crl_policy_act(crl_policy *p, const uint8_t *frame_dev, int64_t frame_stride, int32_t *actions_dev,
                   int64_t action_stride, float *logits_dev, void *stream);
/* The stack as the model sees it: u8 [N, 4, 42, 42], oldest plane first (tests, checkpoints). */
int crl_policy_get_stack(crl_policy *p, uint8_t *stack_out_dev, void *stream);
int crl_policy_set_stack(crl_policy *p, const uint8_t *stack_in_dev, void *stream);
/* Policy.compute_action(obs, deterministic=False) (policy_serving.py:48-56) for crl_policy_act, light and full: from now on the action
 * of env i is drawn by "sampled actions" (below, beside "league draws") with gid = env_id_base + i, key `seed` and n = the number of
 * crl_policy_act calls since THIS call (the counter starts over).  temperature 0 and epsilon 0 is the argmax again; a policy that
 * never had this called plays the argmax.  Refuses (CRL_EINVAL, before any GPU call) what crl_sampling_set_agent refuses. */
int crl_policy_set_sampling(crl_policy *p, float temperature, float epsilon, uint64_t seed, int64_t env_id_base);

/* ---- rollout heads: serving a LEARNER ---------------------------------------------------------
 * The reference's trainers run their own network through trainer.compute_action(obs, deterministic) -> (values, actions, log_probs)
 * (utils/utils.py:121-123) on a FrameStackTensor that step_envs zeroes for finished envs before the next frame is pushed
 * (FrameStackTensor.update(obs, mask), utils/utils.py:158-170, :43-58), and the network changes after every update.  A crl_policy
 * serves such a network with four additions; none of them changes what crl_policy_act computes.
 *
 * Critic.  LightActorCritic.forward / ActorCritic.forward return (logits, value) (utils/network.py:40-47, 83-89):
 * value = critic_linear(features), [1, 1600] + [1] for the light network and [1, 256] + [1] for the full-size one, on the features
 * the actor reads.  crl_policy_set_critic uploads the head (host pointers, torch layout; synchronous like create).  A policy that
 * never got one behaves as before.  On the device the light network's value is summed in a fixed shape of its own (the four
 * channel groups of a position, four neighbouring positions, then the env's 25 such blocks), the full-size one's like a logit: an
 * env's value does not depend on the batch size or on where the env sits in it. */
int crl_policy_set_critic(crl_policy *p, const float *critic_w_host /*[1,1600] or [1,256]*/, const float *critic_b_host /*[1]*/);
/* crl_policy_act plus:
 *   reset_dev   optional u8 [N]: for every env with a non-zero byte all four planes of the stack are zeroed BEFORE this call's frame
 *               is pushed -- the network then sees [0, 0, 0, frame], FrameStackTensor.update with mask = 1 - reset.  One more
 *               launch in front of the act launch on the same stream; with NULL there is none.
 *   values_dev  optional float32 [N]: critic_linear(features) of the same forward pass.
 *   logp_dev    optional float32 [N]: the log-probability of the action THIS call writes to actions_dev, by the rule below.
 * With values_dev and logp_dev both NULL the launches are crl_policy_act's own.  The call advances the same counter as crl_policy_act
 * (the n of "sampled actions") and pushes the same ring; the two may be mixed call by call, and logits and actions are the same
 * bits either way.  Refuses (CRL_EINVAL, before any GPU call) what crl_policy_act refuses, and values_dev on a policy without a
 * critic.
 *
 * Log-probability rule (tests restate it in numpy: rules.rollout_logp_reference).  float32, one rounding per operation; the terms are
 * those of step 3 of "sampled actions" and are formed once for the draw and the log-probability both:
 *   inv_t = the policy's float32 1 / temperature, and 1.0f at temperature 0;
 *   z_a = l_a * inv_t,  m = max z,  d_a = z_a - m,  e_a = expf(d_a),  S = (e0 + e1) + e2,
 *   logp = d_action - logf(S)          (expf, logf: the device library's)
 * `action` is the action written, whether the argmax, the draw or the explore branch chose it.  Epsilon is NOT folded into the
 * probability: logp is the log of softmax(l * inv_t)[action], not of the epsilon-mixed distribution the actions follow. */
int crl_policy_act_rollout(crl_policy *p, const uint8_t *frame_dev, int64_t frame_stride, const uint8_t *reset_dev, int32_t *actions_dev,
                           int64_t action_stride, float *logits_dev, float *values_dev, float *logp_dev, void *stream);
/* Replaces the weights in place, ordered on `stream`: act calls enqueued on it before this call use the old weights, calls after it
 * the new ones; nothing synchronises the device.  Tensors as for crl_policy_create / _create_full (host pointers, torch layouts):
 * conv3_w_host / conv3_b_host are the full-size network's and must be NULL for a LightActorCritic policy.  The critic pair is
 * optional: NULL keeps the current critic.  The tensors are packed into one pinned host buffer that the policy keeps and reuses, and
 * the host pointers are free again when the call returns; a second reload first waits (on the host, on an event) until the first
 * one's copy has left that buffer.  The ring, its head, the play style and its counter are untouched.  Act calls on ANOTHER
 * stream are the caller's to order. */
int crl_policy_load_weights(crl_policy *p, const float *conv1_w_host, const float *conv1_b_host, const float *conv2_w_host,
                            const float *conv2_b_host, const float *conv3_w_host /* full-size only, else NULL */,
                            const float *conv3_b_host /* full-size only, else NULL */, const float *actor_w_host,
                            const float *actor_b_host, const float *critic_w_host /* optional */, const float *critic_b_host /* optional */,
                            void *stream);

/* ---- league: per-env opponents of cPongTournament-v0 on the device --------------------------
 * Stands in for what a POPULATION of the reference's workers does together: each worker's TournamentEnvWrapper draws an opponent
 * of its own (pong/competitive_pong_env.py:27-33 reset_opponent -> random.choice(agent_names)) out of RANDOM (np.random.randint(3),
 * pong/builtin_policies.py:51-58), RULE_BASED (the cheat code, :44-48) and LightActorCritic checkpoints (:61-91,
 * utils/policy_serving.py:46-66).  Here one batch holds the population: `assignment` is an int32 per env on the device (index
 * into the pool, in the order the agents were added), and neither a draw nor an opponent's action touches the host.
 *
 * History: the league owns ONE ring of the last four 42x42 opponent-view frames per env, in crl_policy's layout and with its rule
 * (never cleared at episode ends, one head for all envs).  Every crl_league_act pushes every env's frame, whichever agent the env
 * is assigned to; every CNN agent reads that ring.  With an assignment that never changes, an env's actions are
 * those of a crl_policy of that agent fed the same frames.
 *
 * League draws (tests restate this in numpy; it does not depend on how a batch is cut into shards):
 *   x = Philox4x32-10(counter = (gid & 0xFFFFFFFF, gid >> 32, n, domain), key = (seed & 0xFFFFFFFF, seed >> 32)), word 0 of the
 *   result; gid = env_id_base + i, the env's GLOBAL id; the same round function, multipliers (0xD2511F53, 0xCD9E8D57) and key
 *   increments (0x9E3779B9, 0xBB67AE85) as the serve sampler, whose domain word is 0x504F4E47.
 *   value = (uint64(x) * m) >> 32      -- an integer in [0, m)
 *   opponent of env i: domain = CRL_LEAGUE_DOMAIN_OPPONENT, m = agents in the pool, n = the number of opponent draws env i has had
 *                      since crl_league_create / crl_league_seed (a per-env counter; 0 for the first draw);
 *   RANDOM's action:   domain = CRL_LEAGUE_DOMAIN_ACTION, m = 3, n = the number of crl_league_act calls since create / seed
 *                      (0 for the first call; drawn only for envs assigned to RANDOM, the counter moves for all).
 * RANDOM is therefore another stream than the reference's np.random.
 *
 * Sampled actions (tests restate this in numpy: league_sample_reference; same generator, key and gid as "league draws").  Every agent
 * of a pool, and every crl_policy, carries a play style: temperature (float32, >= 0; 0 = greedy, the default) and epsilon (in
 * [0, 1], default 0).  Policy.compute_action(obs, deterministic=False) (utils/policy_serving.py:48-56) samples from
 * Categorical(logits); here the lane that writes env i's action draws it in the kernel's epilogue, nothing touches the host.  At act
 * call n (the counter of RANDOM's action: crl_league_act / crl_policy_act calls since create / seed, 0 for the first) ONE Philox call
 * with counter (gid lo, gid hi, n, CRL_LEAGUE_DOMAIN_SAMPLE) gives the words x0, x1, x2:
 *   1. explore:  eps_q = min(floor(epsilon * 2^32), 0xFFFFFFFF), computed on the host in double from the float32 epsilon.  If
 *                x1 < eps_q the action is (uint64(x2) * 3) >> 32.  RULE_BASED plays the cheat code when it does not explore; epsilon
 *                (and temperature) have no effect on RANDOM, temperature has none on RULE_BASED.
 *   2. greedy:   otherwise, with temperature == 0: the argmax of the logits, first index on ties.
 *   3. sample:   otherwise, in float32 with one rounding per operation: z_a = l_a * inv_t (inv_t = float32 1 / temperature, divided
 *                once on the host), m = max z, e_a = exp(z_a - m), S = (e0 + e1) + e2, r = float(x0 >> 8) * 2^-24 (exact, in
 *                [0, 1)); action 0 if r * S < e0, 1 if r * S < e0 + e1, else 2.  (`exp` is the device library's expf; a draw whose r
 *                lies within its error of a boundary may fall on either side.)
 * The logits written to logits_dev are the raw l_a whatever the style.
 *
 * Full-size agents.  A pool also holds agents of kind CRL_POOL_KIND_FULL: the full-size ActorCritic (utils/network.py:14-56, the
 * network of crl_policy_create_full; what Policy(..., use_light_model=False) serves), added with crl_pool_add_full.  Such an agent
 * reads the league's shared ring like every CNN agent, has a list of its envs, takes its play style from crl_sampling_set_agent,
 * and its rows of logits_dev are written.  Its forward pass is crl_policy_act's for the same frames, bit for bit, whatever envs the
 * list holds and in whatever order.
 *   scratch: the activations between its three kernels (15 488 + 1 024 bytes per row, 16.5 KB) live in ONE scratch per league of
 *            scratch_rows rows, shared by all full-size agents of the pool (their launches are ordered on the stream) and allocated
 *            by the first crl_pool_add_full.  scratch_rows = 0 means min(num_envs, 65 536): at 65 536 rows that is about 1.1 GB.
 *            Each agent's weights take 3.96 MB more.
 *   passes:  the agent's env count is known on the device only, so every crl_league_act enqueues ceil(num_envs / scratch_rows)
 *            passes of three launches per full-size agent; pass p serves positions [p * scratch_rows, min(count, (p + 1) *
 *            scratch_rows)) of the list, a pass past the count returns at once.
 *   sampled actions: drawn with gid = env_id_base + i of the ENV i the row belongs to, not with the row's place in the list.
 * (The kind is a #define and the entry point is named crl_pool_*: the kind enum and the thirteen crl_league_* entry points stay
 * what they were.) */
#define CRL_LEAGUE_MAX_AGENTS 16
#define CRL_LEAGUE_DOMAIN_OPPONENT 0x4C47554Fu /* "LGUO" */
#define CRL_LEAGUE_DOMAIN_ACTION 0x4C475541u   /* "LGUA" */
#define CRL_LEAGUE_DOMAIN_SAMPLE 0x4C475553u   /* "LGUS" */
enum crl_league_kind { CRL_LEAGUE_RANDOM = 0, CRL_LEAGUE_RULE_BASED = 1, CRL_LEAGUE_LIGHT = 2 };
#define CRL_POOL_KIND_FULL 3 /* a full-size ActorCritic agent ("full-size agents" above); not a value crl_league_add_builtin takes */
typedef struct crl_league crl_league;
/* TournamentEnvWrapper.__init__ (competitive_pong_env.py:10-25) for num_envs envs whose global ids start at env_id_base; the pool is
 * empty, every env is assigned agent 0. */
int crl_league_create(int32_t device, int64_t num_envs, int64_t env_id_base, uint64_t seed, crl_league **out);
void crl_league_destroy(crl_league *l);
/* get_compute_action_function("RANDOM" / "RULE_BASED") (builtin_policies.py:61-91): appends the agent to the pool. */
int crl_league_add_builtin(crl_league *l, int32_t kind);
/* get_compute_action_function("WEAK" / "MEDIUM") or a LightActorCritic checkpoint of the caller's (builtin_policies.py:68-83,
 * utils/network.py:73-93): appends the agent; weights as for crl_policy_create. */
int crl_league_add_light(crl_league *l, const float *conv1_w_host /*[16,4,4,4]*/, const float *conv1_b_host /*[16]*/,
                         const float *conv2_w_host /*[16,16,2,2]*/, const float *conv2_b_host /*[16]*/,
                         const float *actor_w_host /*[3,1600]*/, const float *actor_b_host /*[3]*/);
/* A full-size ActorCritic checkpoint of the caller's ("full-size agents" above): appends the agent with kind CRL_POOL_KIND_FULL; weights
 * (host pointers, torch layouts) as for crl_policy_create_full.  scratch_rows: rows of the league's shared activation scratch, 0 =
 * min(num_envs, 65 536); the first full-size agent fixes it, a later one passes 0 or the same value.  Refuses (CRL_EINVAL, before
 * any GPU call) a null league or weight pointer, a negative scratch_rows, a full pool and a scratch_rows other than the league's. */
int crl_pool_add_full(crl_league *l, const float *conv1_w_host /*[16,4,4,4]*/, const float *conv1_b_host /*[16]*/,
                      const float *conv2_w_host /*[32,16,4,4]*/, const float *conv2_b_host /*[32]*/,
                      const float *conv3_w_host /*[256,32,11,11]*/, const float *conv3_b_host /*[256]*/,
                      const float *actor_w_host /*[3,256]*/, const float *actor_b_host /*[3]*/, int64_t scratch_rows);
/* crl_policy_load_weights for slot `agent` of a pool: a learner's newer snapshot replaces the weights of a CNN agent in place (the
 * slot's device blob), ordered on `stream` like that call and through a pinned staging buffer of the league's own; a pool of
 * CRL_LEAGUE_MAX_AGENTS append-only slots can so follow a learner for ever.  Tensors as for crl_league_add_light / crl_pool_add_full.
 * Assignment, lists, play styles, the shared ring and the scratch are untouched.  Refuses (CRL_EINVAL, before any GPU call) a null
 * argument, a slot outside the pool, a built-in slot and a slot of the other kind.  (Named crl_pool_* like crl_pool_add_full: the
 * crl_league_* surface stays the thirteen entry points it was.) */
int crl_pool_load_light(crl_league *l, int32_t agent, const float *conv1_w_host /*[16,4,4,4]*/, const float *conv1_b_host /*[16]*/,
                        const float *conv2_w_host /*[16,16,2,2]*/, const float *conv2_b_host /*[16]*/,
                        const float *actor_w_host /*[3,1600]*/, const float *actor_b_host /*[3]*/, void *stream);
int crl_pool_load_full(crl_league *l, int32_t agent, const float *conv1_w_host /*[16,4,4,4]*/, const float *conv1_b_host /*[16]*/,
                       const float *conv2_w_host /*[32,16,4,4]*/, const float *conv2_b_host /*[32]*/,
                       const float *conv3_w_host /*[256,32,11,11]*/, const float *conv3_b_host /*[256]*/,
                       const float *actor_w_host /*[3,256]*/, const float *actor_b_host /*[3]*/, void *stream);
/* The play style of agent `agent` of the pool ("sampled actions" above), from the next crl_league_act on; host values, no GPU call.
 * Refuses (CRL_EINVAL) an agent outside the pool, a negative or non-finite temperature (or one so small that 1 / temperature is no
 * float32) and an epsilon outside [0, 1].  An agent at (0, 0) is served by the launch it always had.  (Named crl_sampling_*: the
 * crl_league_* surface stays the thirteen entry points it was.) */
int crl_sampling_set_agent(crl_league *l, int32_t agent, float temperature, float epsilon);
int crl_sampling_get_agent(crl_league *l, int32_t agent, float *temperature, float *epsilon);
/* TournamentEnvWrapper.seed's share for the draws (competitive_pong_env.py:50-51): new key, all draw counters back to 0. */
int crl_league_seed(crl_league *l, uint64_t seed, void *stream);
/* reset_opponent(agent_name) (competitive_pong_env.py:27-33) per env: ids_dev int32 [N] on the device (each in [0, agents); an id
 * outside plays RULE_BASED and is in nobody's list), or ids_dev = NULL and agent `all` for every env.  Rebuilds counts and lists. */
int crl_league_set_assignment(crl_league *l, const int32_t *ids_dev, int32_t all, void *stream);
int crl_league_get_assignment(crl_league *l, int32_t *ids_out_dev, void *stream);
/* reset_opponent() without a name (competitive_pong_env.py:28-29), once per env: a fresh league draw for every env whose byte in
 * done_dev [N] is non-zero, or for every env when done_dev is NULL.  Rebuilds counts and lists.  No host synchronisation. */
int crl_league_resample(crl_league *l, const uint8_t *done_dev, void *stream);
/* Debug / tests: counts_out_dev int32 [CRL_LEAGUE_MAX_AGENTS] (envs per agent); lists_out_dev optional int32 [agents][N]: row a
 * holds the env indices of CNN agent a (LightActorCritic or full-size) in its first counts[a] entries (in no particular order),
 * other rows are left as they are. */
int crl_league_get_lists(crl_league *l, int32_t *counts_out_dev, int32_t *lists_out_dev, void *stream);
/* TournamentEnvWrapper.step's opponent half (competitive_pong_env.py:35-41 `self.current_agent(self.prev_opponent_obs)`), per env:
 * pushes env i's frame (frame_dev + i * frame_stride, as crl_policy_act) onto the shared ring and writes the action of the env's
 * agent to actions_dev[i * action_stride].  logits_dev: optional float32 [N, 3]; rows of envs on RANDOM / RULE_BASED are left as
 * they are. */
int crl_league_act(crl_league *l, const uint8_t *frame_dev, int64_t frame_stride, int32_t *actions_dev, int64_t action_stride,
                   float *logits_dev, void *stream);
/* Policy.reset (policy_serving.py:46-47) for the shared ring; the stack as crl_policy_get_stack / _set_stack hand it over. */
int crl_league_reset(crl_league *l, void *stream);
int crl_league_get_stack(crl_league *l, uint8_t *stack_out_dev, void *stream);
int crl_league_set_stack(crl_league *l, const uint8_t *stack_in_dev, void *stream);

/* ---- league ledger: per-opponent results and win-rate-weighted opponent draws on the device ---
 * What a league trainer keeps beside a crl_league (an object of its own; crl_league_* knows nothing of it): how the learner fares
 * against every agent of the pool, and a draw of the next opponent that is weighted by it (prioritised fictitious self-play).
 * All work is ordered on the caller's stream; no call synchronises with the host, the getters hand over device memory.
 *
 * State.  Per env: ret int32 (sum of the learner's step rewards in the running episode), len int32 (its steps), draw_ctr uint32
 * (the ledger's own draw counter).  Per agent (CRL_LEAGUE_MAX_AGENTS rows): CRL_LEDGER_COUNTERS int64 counters, laid out
 * [counter][agent] in the order of enum crl_ledger_counter; one int64 `ignored`.  A weight table uint32 w[CRL_LEAGUE_MAX_AGENTS]
 * (1 for every agent of the pool after create, 0 beyond the pool).
 *
 * crl_ledger_step, one launch with one lane per env:
 *   1. ret += (int)reward[i * reward_stride]; len += 1  (Pong's step rewards are integers held in float32);
 *   2. where done[i] != 0 the episode is credited to assign[i], the agent that PLAYED it: episodes += 1, one of wins (ret > 0) /
 *      losses (ret < 0) / draws (ret == 0) += 1, return_sum += ret, length_sum += len; then ret = len = 0.  An id outside
 *      [0, agents) is credited nowhere and counted in `ignored`.  All sums are 64-bit integers, so the totals do not depend on
 *      the order in which wavefronts arrive;
 *   3. ids_out[i] = assign[i], replaced by a ledger draw where done[i] != 0 and redraw != 0 (draw_ctr[i] += 1 there).
 *      ids_out may be assign itself.
 *
 * Ledger draws (tests restate this in numpy; beside "league draws" above, same generator and key):
 *   x = word 0 of Philox4x32-10(counter = (gid & 0xFFFFFFFF, gid >> 32, n, CRL_LEDGER_DOMAIN_OPPONENT), key = seed),
 *   gid = env_id_base + i, n = draw_ctr[i] (0 for an env's first draw since crl_ledger_create / crl_ledger_seed);
 *   T = sum of w[a] over the table, 0 < T < 2^32;  r = (uint64(x) * T) >> 32  -- an integer in [0, T);
 *   the drawn agent is the smallest a with w[0] + ... + w[a] > r.  An agent of weight 0 is never drawn.
 * A draw depends on (seed, global env id, counter, table) alone: shards that hold the same table draw what the whole batch would.
 * crl_ledger_set_weights refuses a table with T == 0 or T >= 2^32.  crl_ledger_pfsp_weights cannot look at its result without a
 * synchronisation: it refuses a floor with which agents * (floor + 65535) reaches 2^32, and should a table made with floor = 0
 * sum to 0, a step keeps the assignment of the envs it would have redrawn and leaves their draw_ctr alone.
 *
 * PFSP weights (one wavefront; float64, one rounding per operation, numpy reproduces them bit for bit), agent a < agents:
 *   p = ((wins + 0.5 * draws) + 1.0) / (episodes + 2.0)       -- 0.5 for an agent that was never played
 *   CRL_LEDGER_PFSP_HARD:     f = (1 - p)^k, k = exponent >= 1, as k - 1 multiplications f = f * (1 - p) from f = 1 - p
 *   CRL_LEDGER_PFSP_VARIANCE: f = p * (1 - p)                  (exponent is not used)
 *   w[a] = floor + (uint32)floor(f * 65535.0);  w[a] = 0 for a >= agents. */
#define CRL_LEDGER_DOMAIN_OPPONENT 0x4C475557u /* "LGUW" */
#define CRL_LEDGER_COUNTERS 6
enum crl_ledger_counter { CRL_LEDGER_EPISODES = 0, CRL_LEDGER_WINS = 1, CRL_LEDGER_LOSSES = 2, CRL_LEDGER_DRAWS = 3,
                          CRL_LEDGER_RETURN_SUM = 4, CRL_LEDGER_LENGTH_SUM = 5 };
enum crl_ledger_pfsp { CRL_LEDGER_PFSP_HARD = 0, CRL_LEDGER_PFSP_VARIANCE = 1 };
typedef struct crl_ledger crl_ledger;
/* A ledger for num_envs envs whose global ids start at env_id_base and a pool of `agents` (1..CRL_LEAGUE_MAX_AGENTS) agents. */
int crl_ledger_create(int32_t device, int64_t num_envs, int64_t env_id_base, uint64_t seed, int32_t agents, crl_ledger **out);
void crl_ledger_destroy(crl_ledger *l);
/* New key for the draws, every draw_ctr back to 0 (results and weights stay). */
int crl_ledger_seed(crl_ledger *l, uint64_t seed, void *stream);
/* Zeroes the counters, `ignored` and every env's ret / len (weights, key and draw counters stay). */
int crl_ledger_reset(crl_ledger *l, void *stream);
/* The pool grew or shrank: rows that enter the pool get weight 1, rows that leave it weight 0; counters stay. */
int crl_ledger_set_agents(crl_ledger *l, int32_t agents, void *stream);
/* w_host: uint32 [count] on the HOST, count == agents (read before the call returns; the table changes in stream order). */
int crl_ledger_set_weights(crl_ledger *l, const uint32_t *w_host, int32_t count, void *stream);
/* w_out_dev: uint32 [CRL_LEAGUE_MAX_AGENTS] on the device. */
int crl_ledger_get_weights(crl_ledger *l, uint32_t *w_out_dev, void *stream);
/* Fills the weight table by the PFSP rule above from counters_dev (int64 [CRL_LEDGER_COUNTERS][CRL_LEAGUE_MAX_AGENTS] on the
 * device, e.g. counters all-reduced over the shards so that every rank holds the same table), or from the ledger's own counters
 * when counters_dev is NULL. */
int crl_ledger_pfsp_weights(crl_ledger *l, const int64_t *counters_dev, int32_t mode, int32_t exponent, uint32_t floor, void *stream);
/* Counters as int64 [CRL_LEDGER_COUNTERS][CRL_LEAGUE_MAX_AGENTS] and `ignored` as int64 [1] (optional), device memory. */
int crl_ledger_get_counters(crl_ledger *l, int64_t *counters_out_dev, int64_t *ignored_out_dev, void *stream);
int crl_ledger_set_counters(crl_ledger *l, const int64_t *counters_dev, const int64_t *ignored_dev, void *stream);
/* Checkpoints / tests: the per-env values, each [N] on the device, each optional. */
int crl_ledger_get_env_state(crl_ledger *l, int32_t *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev, void *stream);
int crl_ledger_set_env_state(crl_ledger *l, const int32_t *ret_dev, const int32_t *len_dev, const uint32_t *draw_ctr_dev, void *stream);
/* The per-step call described above.  assign_dev int32 [N] (crl_league_get_assignment's copy, taken BEFORE any redraw);
 * reward_dev float32, env i at reward_dev[i * reward_stride] (the env's reward buffer, column 0: stride 2 for cPongDouble);
 * done_dev uint8 [N]; ids_out_dev int32 [N] (for crl_league_set_assignment). */
int crl_ledger_step(crl_ledger *l, const int32_t *assign_dev, const float *reward_dev, int64_t reward_stride, const uint8_t *done_dev,
                    int32_t redraw, int32_t *ids_out_dev, void *stream);

/* ---- arena: every agent of a pool against every other, both seats served, pair results on the device ---
 * Stands in for evaluate_two_policies_in_batch (pong/evaluate.py:6-88) called once for every pair of a pool: the reference plays
 * ONE pair of policies per call and the host walks every step.  Here one batch holds the whole round-robin: env i plays the pair
 * (pairs[2i], pairs[2i+1]) = (left agent, right agent), both indices into a pool of up to CRL_LEAGUE_MAX_AGENTS agents.  Serving the
 * two bats is a crl_league of 2N virtual envs (virtual env 2i + seat; its int32 [2N] assignment IS the array of pairs); the arena
 * is an object beside it, as crl_ledger is: crl_arena_* never reaches into a league, the caller passes the pairs in and takes the
 * next pairs out.  All work is ordered on the caller's stream; no call synchronises with the host.
 *
 * State.  Per env: ret int32 (sum of the LEFT agent's step rewards in the running episode), len int32 (its steps), draw_ctr uint32.
 * Per cell (CRL_LEAGUE_MAX_AGENTS^2 cells, cell = left * 16 + right): CRL_ARENA_COUNTERS int64 counters, laid out [counter][cell]
 * in the order of enum crl_arena_counter; one int64 `ignored`.  A weight table uint32 w[16][16] (after create: 1 for every
 * off-diagonal cell of the pool, 0 elsewhere).
 *
 * Arena books -- crl_arena_step, one launch with one lane per env:
 *   1. ret += (int)reward[i * reward_stride]; len += 1  (the left agent's reward: column 0 of the env's reward buffer, stride 2);
 *   2. where done[i] != 0 the episode goes to cell (pairs[2i], pairs[2i+1]), the pair that PLAYED it: episodes += 1, one of
 *      left_wins (ret > 0) / right_wins (ret < 0) / draws (ret == 0) += 1, return_sum += ret, length_sum += len; then ret = len = 0.
 *      If either id is outside [0, agents) nothing is booked to a cell and `ignored` is counted.  All sums are 64-bit integers, so
 *      the totals do not depend on the order in which wavefronts arrive;
 *   3. pairs_out[2i], pairs_out[2i+1] = the pair played, replaced by an arena draw where done[i] != 0 and redraw != 0
 *      (draw_ctr[i] += 1 there).  pairs_out may be pairs itself.  A table that sums to 0 keeps the pair and leaves the counter alone.
 *
 * Arena draws (tests restate this in numpy; beside "league draws" above, same generator and key):
 *   x = word 0 of Philox4x32-10(counter = (gid & 0xFFFFFFFF, gid >> 32, n, CRL_ARENA_DOMAIN_PAIR), key = seed),
 *   gid = env_id_base + i, the REAL env's global id (not a virtual env's), n = draw_ctr[i];
 *   T = sum of all 256 weights, 0 < T < 2^32;  r = (uint64(x) * T) >> 32  -- an integer in [0, T);
 *   the drawn cell is the smallest row-major index c = left * 16 + right whose cumulative weight w[0] + ... + w[c] exceeds r (the
 *   kernel walks the 16 row sums and then the row: the same cell in 32 steps).  A cell of weight 0 is never drawn.
 * A draw depends on (seed, global env id, counter, table) alone: shards that hold the same table draw what the whole batch would.
 *
 * Balance weights (one workgroup, one lane per cell; integers only, numpy reproduces them exactly): over the SCHEDULED cells -- left
 * and right in the pool, left != right unless include_mirror -- e = EPISODES[cell], m = the largest e;
 *   w[cell] = floor + min(m - e, 65535) for a scheduled cell, 0 for every other.
 * Pairs played less are drawn more; with floor >= 1 every scheduled pair stays reachable.  The call refuses a floor with which
 * agents^2 * (floor + 65535) reaches 2^32. */
#define CRL_ARENA_DOMAIN_PAIR 0x4C475550u /* "LGUP" */
#define CRL_ARENA_COUNTERS 6
enum crl_arena_counter { CRL_ARENA_EPISODES = 0, CRL_ARENA_LEFT_WINS = 1, CRL_ARENA_RIGHT_WINS = 2, CRL_ARENA_DRAWS = 3,
                         CRL_ARENA_RETURN_SUM = 4, CRL_ARENA_LENGTH_SUM = 5 };
typedef struct crl_arena crl_arena;
/* The books of evaluate_two_policies_in_batch (pong/evaluate.py:6-88) for every pair of a pool at once: num_envs envs whose global
 * ids start at env_id_base, a pool of `agents` (1..CRL_LEAGUE_MAX_AGENTS) agents. */
int crl_arena_create(int32_t device, int64_t num_envs, int64_t env_id_base, uint64_t seed, int32_t agents, crl_arena **out);
void crl_arena_destroy(crl_arena *a);
/* New key for the draws, every draw_ctr back to 0 (results and weights stay). */
int crl_arena_seed(crl_arena *a, uint64_t seed, void *stream);
/* Zeroes the counters, `ignored` and every env's ret / len (weights, key and draw counters stay). */
int crl_arena_reset(crl_arena *a, void *stream);
/* The pool grew or shrank: cells that enter it get weight 1 off the diagonal and 0 on it, cells that leave it weight 0. */
int crl_arena_set_agents(crl_arena *a, int32_t agents, void *stream);
/* w_host: uint32 [agents][agents] on the HOST, count == agents * agents (read before the call returns; the table changes in stream
 * order).  Refuses T == 0 and T >= 2^32. */
int crl_arena_set_weights(crl_arena *a, const uint32_t *w_host, int32_t count, void *stream);
/* w_out_dev: uint32 [CRL_LEAGUE_MAX_AGENTS][CRL_LEAGUE_MAX_AGENTS] on the device. */
int crl_arena_get_weights(crl_arena *a, uint32_t *w_out_dev, void *stream);
/* Fills the table by the balance rule above from counters_dev (int64 [CRL_ARENA_COUNTERS][256] on the device, e.g. counters
 * all-reduced over the shards so that every rank holds the same table), or from the arena's own counters when counters_dev is NULL:
 * the schedule that evens out the episodes per pair which evaluate.py:6-88 gets by being called once per pair. */
int crl_arena_balance_weights(crl_arena *a, const int64_t *counters_dev, int32_t include_mirror, uint32_t floor, void *stream);
/* Counters as int64 [CRL_ARENA_COUNTERS][256] and `ignored` as int64 [1] (optional), device memory: the per-pair totals that
 * evaluate.py:6-88 returns for its one pair. */
int crl_arena_get_counters(crl_arena *a, int64_t *counters_out_dev, int64_t *ignored_out_dev, void *stream);
int crl_arena_set_counters(crl_arena *a, const int64_t *counters_dev, const int64_t *ignored_dev, void *stream);
/* Checkpoints / tests: the per-env values, each [N] on the device, each optional. */
int crl_arena_get_env_state(crl_arena *a, int32_t *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev, void *stream);
int crl_arena_set_env_state(crl_arena *a, const int32_t *ret_dev, const int32_t *len_dev, const uint32_t *draw_ctr_dev, void *stream);
/* A fresh arena draw for EVERY env (draw_ctr += 1 each): pairs_out_dev int32 [2N], which may be pairs_dev; a table that sums to 0
 * hands pairs_dev through.  The choice of the pair to play that a caller of evaluate.py:6-88 makes on the host. */
int crl_arena_draw(crl_arena *a, const int32_t *pairs_dev, int32_t *pairs_out_dev, void *stream);
/* The per-step call described above ("arena books"): the episode accounting of evaluate.py:6-88's loop for every pair at once.
 * pairs_dev int32 [2N] (the pairs that played this step); reward_dev float32, env i at reward_dev[i * reward_stride] (the env's
 * reward buffer, column 0: stride 2 for cPongDouble); done_dev uint8 [N]; pairs_out_dev int32 [2N] (for
 * crl_league_set_assignment of the 2N-virtual-env league). */
int crl_arena_step(crl_arena *a, const int32_t *pairs_dev, const float *reward_dev, int64_t reward_stride, const uint8_t *done_dev,
                   int32_t redraw, int32_t *pairs_out_dev, void *stream);

/* ---- rollout storage: T steps of a learner's rollout on the device, GAE, minibatch gather -------------------
 * Stands in for the storage a PPO / A2C trainer around the reference keeps between trainer.compute_action and its update: per step the
 * stacked observation as FrameStackTensor holds it (float32 [N, 4, 42, 42], utils/utils.py:145-173: 28 224 bytes per env and step), the
 * action, its log-probability, the value, the reward and the done flag; then returns and advantages, then shuffled minibatches.  A step
 * adds ONE new 42 x 42 plane per env -- the other three planes of its stack are the planes of the three steps before it, as in the frame
 * ring of a crl_policy -- so a crl_rollout keeps T + 3 planes per env and rebuilds the stack of a sample when it is gathered.  An
 * object of its own beside crl_policy: the caller hands the act call's inputs and outputs over.  All work is ordered on the caller's
 * stream; no call synchronises with the host except crl_rollout_stats.  crl_rollout_create, _destroy and _stats make the storage's
 * device current themselves; every other call launches on the device that is current, so the caller has the storage's device current
 * (as it has for the stream it passes).
 *
 * State (num_steps = T, num_envs = N, T * N < 2^31).  planes u8 [T + 3][N][1776]: a plane padded to 111 16-byte chunks as in the ring,
 * step-major; row t + 3 is the frame pushed at step t, rows 0..2 the three frames before step 0, oldest first.  Per step and env:
 * reset u8, depth u8, action int32, log-prob, value, reward, advantage and return float32, done u8.  Per env: depth_carry u8.
 * Two float64 statistics.
 *
 * Stack rule (tests restate it in numpy: rules.rollout_stack_reference).  depth[t][e] is the number of planes of the stack of step t
 * that are not masked, 1..4:
 *   depth[t][e] = reset[t][e] ? 1 : min(4, depth[t-1][e] + 1);
 *   depth[-1][e] = 3 after crl_rollout_begin with a stack and on a fresh object (whose history rows are zero): those rows are
 *   physically what the ring held; after a carrying crl_rollout_begin it is min(3, depth[T-1][e]) of the rollout before.
 *   Plane j (0 = the oldest) of sample (t, e) is row t + j of env e if 3 - j < depth[t][e], else all zeros.
 * So the gathered stack of (t, e) is, byte for byte, what crl_policy_get_stack gave for env e right after the crl_policy_act_rollout call
 * of step t with the same frames and reset flags: FrameStackTensor.update(obs, 1 - reset), utils/utils.py:158-170.
 *
 * GAE rule (tests restate it: rules.gae_reference).  One lane per env, float32 with one rounding per operation, no contraction;
 * g = float32(gamma), gl = g * float32(lam) in float32, both formed once on the host:
 *   acc = 0;  for t = T-1 .. 0:
 *     nd = done[t] ? 0.0f : 1.0f;   vnext = (t == T-1) ? last_values : values[t+1];
 *     delta = (rewards[t] + (g * vnext) * nd) - values[t];   acc = delta + (gl * nd) * acc;
 *     adv[t] = acc;   ret[t] = acc + values[t].
 *
 * Statistics (when crl_rollout_finish is asked to normalise).  Mean and unbiased standard deviation of all T * N advantages in float64,
 * two passes: mean = sum(x) / (T * N), then std = sqrt(sum((x - mean)^2) / (T * N - 1)), and std = 0 where T * N = 1 (the one
 * advantage then normalises to (adv - mean32) / 1e-5f = 0).  Each sum has a fixed shape: workgroup w of
 * G = min(256, ceil(T * N / 256)) adds elements w * 256 + lane, + G * 256, ... in order, its 256 lanes' sums go through a binary tree,
 * and one final workgroup adds the G partial sums through the same tree.  No floating-point atomics: two runs give the same bits.
 * A gathered advantage is then (adv - mean32) / (std32 + 1e-5f) in float32 with a true division, mean32 and std32 the float32
 * roundings of the two statistics; without normalisation it is adv. */
typedef struct crl_rollout crl_rollout;
int crl_rollout_create(int32_t device, int64_t num_envs, int64_t num_steps, crl_rollout **out);
void crl_rollout_destroy(crl_rollout *r);
/* Starts a rollout: step 0 is recorded next.  stack_dev: u8 [N][4][42][42] as crl_policy_get_stack writes it, taken BEFORE the act call
 * of step 0: its planes 1..3 become the history rows (plane 0 is the one that call rolls out).  NULL carries over: the last three rows
 * and the depths of the finished rollout become the history (on a fresh object: zero rows at depth 3), so a rollout that continues the
 * one before gathers what an uninterrupted one would.  Refuses (CRL_EINVAL) to carry over from a rollout that is not finished. */
int crl_rollout_begin(crl_rollout *r, const uint8_t *stack_dev, void *stream);
/* Step t, one launch: the inputs and outputs of its crl_policy_act_rollout call.  frame_dev / frame_stride: as that call took them
 * (stride a multiple of 4 and >= 1764, pointer 4-byte aligned); reset_dev u8 [N] or NULL (no env flagged); actions_dev int32, env i
 * at actions_dev[i * action_stride]; values_dev, logp_dev float32 [N].  actions, values and log-probs are each optional: NULL stores
 * zeros.  t must be the next step: 0 after begin (or on a fresh object), then 1, 2, ... T - 1. */
int crl_rollout_record(crl_rollout *r, int64_t t, const uint8_t *frame_dev, int64_t frame_stride, const uint8_t *reset_dev,
                       const int32_t *actions_dev, int64_t action_stride, const float *values_dev, const float *logp_dev, void *stream);
/* What the env answered to step t's actions: rewards_dev float32, env i at rewards_dev[i * reward_stride] (the learner's column of
 * the env's (N, 2) reward buffer: stride 2); done_dev u8 [N] (any non-zero byte is a done).  In step order, each after its record. */
int crl_rollout_outcome(crl_rollout *r, int64_t t, const float *rewards_dev, int64_t reward_stride, const uint8_t *done_dev, void *stream);
/* After T outcomes: advantages and returns by the GAE rule; last_values_dev float32 [N] = the values of the observation after the last
 * step (NULL: zeros); with normalize != 0 the statistics too.  May be called again (other gamma / lam) before the next begin. */
int crl_rollout_finish(crl_rollout *r, const float *last_values_dev, double gamma, double lam, int32_t normalize, void *stream);
/* A minibatch, one wavefront per sample: idx_dev int64 [B] on the device, flat indices t * N + e in any order, duplicates allowed.
 * obs_out_dev: [B][4][42][42] as CRL_OBS_F32 (values 0..255, 16-byte aligned) or CRL_OBS_U8 (4-byte aligned), the stack by the stack
 * rule; actions_out_dev int32 [B]; logp / values / returns / adv float32 [B], adv normalised if the finish was.  Every output is
 * optional (NULL).  The validity of the indices is the caller's, as with every device-side index array of this header. */
int crl_rollout_gather(crl_rollout *r, const int64_t *idx_dev, int64_t count, void *obs_out_dev, int32_t obs_dtype, int32_t *actions_out_dev,
                       float *logp_out_dev, float *values_out_dev, float *returns_out_dev, float *adv_out_dev, void *stream);
/* out2_host[0] = mean, [1] = std of the advantages, after a finish that normalises.  Synchronises the device (tests, logging). */
int crl_rollout_stats(crl_rollout *r, double *out2_host);
/* The host-side state machine refuses, with CRL_EINVAL and before any GPU call: a record whose t is not the next step or that follows a
 * finish without a begin; an outcome without its record or out of step order; a finish before T outcomes; a gather before the finish;
 * statistics that were not computed; a carrying begin on an unfinished rollout; null or misaligned pointers.  A refused call changes
 * nothing. */

/* ---- ppo update: the learner's gradient and optimiser step for the LightActorCritic on the device ----------------
 * Closes the loop between crl_rollout_gather and crl_policy_load_weights: a crl_ppo holds a learner's master weights (float32, the
 * policy blob: conv1 [16,4,4,4] | b1 [16] | conv2 [16,16,2,2] | b2 [16] | actor [3,1600] | ba [3] + 1 pad | critic [1,1600] | bc [1] + 3
 * pads = 8 488 floats, 8 484 of them parameters) and Adam's two moments, computes the gradient of the loss below over a minibatch
 * of a FINISHED crl_rollout straight from its stored uint8 planes, and steps.  The reference ships no trainer (utils/network.py has
 * only the networks), so the loss is defined HERE; tests restate it with autograd in float64 (rules.ppo_loss_reference) and the
 * optimiser in numpy float32 (rules.adam_reference).  All work is ordered on the caller's stream; only crl_ppo_create, _set_weights,
 * _get_weights, _stats and a crl_ppo_get_grad that copies synchronise.  The caller has the learner's device current.
 *
 * Loss, per sample (stack = the sample's uint8 stack by the stack rule above, action, old_logp, ret as stored, A = the advantage as
 * crl_rollout_gather hands it out: normalised if the finish normalised).  Every comparison is part of the rule:
 *   x = stack / 255;  z1 = conv1(x) + b1 (4 x 4, stride 2: 16 x 20 x 20),  a1 = max(z1, 0);  z2 = conv2(a1) + b2 (2 x 2, stride 2:
 *   16 x 10 x 10),  a2 = max(z2, 0), flattened channel-major to 1600 features;  logits = actor(a2),  v = critic(a2);
 *   the ReLU's derivative is z > 0 ? 1 : 0;
 *   logp_k = log_softmax(logits)_k,  p_k = exp(logp_k),  logp = logp_action.  The temperature is FIXED at 1: a learner whose actions
 *   were drawn at another temperature is out of scope (its stored log-probs would be of another distribution);
 *   r = exp(logp - old_logp);
 *   policy  = -min(r A, clamp(r, 1 - c, 1 + c) A),  so  d policy / d logp = -A r  when (A >= 0 and r < 1 + c) or (A < 0 and r > 1 - c),
 *             and 0 otherwise;
 *   value   = 0.5 (ret - v)^2   (unclipped);
 *   entropy = H = -sum_k p_k logp_k;
 *   loss    = mean over the B samples of (policy + vf * value - ent * entropy).
 * Closed forms the kernel uses:  d loss_b / d logit_k = (d policy / d logp) (1[k = action] - p_k) + ent p_k (logp_k + H),
 * d loss_b / d v = vf (v - ret).  The convolutions are float32; from the features a2 on, the device works in float64 up to dlogits and
 * dv, which are rounded once to float32: logits and v are float64 sums over the float32 features and weights (the head sums are long
 * and cancel, and a sample's whole gradient hangs on v - ret and logp - old_logp), m = max logit, d_k = logit_k - m, e_k = exp(d_k),
 * S = (e0 + e1) + e2, logp_k = d_k - log(S), p_k = e_k / S; c, vf, ent are the float32 values passed, widened.
 * Statistics of a call: the means over the B samples of policy, value, entropy, old_logp - logp (the approximate KL) and of
 * 1[r < 1 - c or r > 1 + c] (the clipped share); each sample's term is formed and summed in float64.
 *
 * Gradient: the exact derivative of `loss` with respect to the eight tensors, float32, in the blob's layout (pads zero).
 * Summation shape -- a function of B alone, not of the device, the grid or any arrival order; no floating-point atomics; the same idx
 * gives the same bits on every run:
 *   groups of 8 consecutive idx entries; W = min(256, ceil(B / 8)) workgroups; workgroup w takes groups w, w + W, w + 2 W, ... in order.
 *   Within a workgroup: a group is 50 tiles of 16 conv2 positions q = 16 t + j (sample q / 100, position q % 100), tile t belongs to
 *   wavefront t % 8.  Conv gradients: a wavefront adds its tiles in order into float32 matrix accumulators (v_mfma_f32_16x16x4_f32,
 *   four positions per step), over all its groups; at the end the eight wavefronts' accumulators are added in wavefront order 0..7.
 *   Conv biases: per-lane float32 sums in the same order, then a butterfly over the lanes.  Head weights: thread f of 512 adds
 *   d_k[e] * a2[e][f] for the group's samples e = 0..7 in order, fused multiply-add, over all its groups; head biases: one thread, same
 *   order.  A logit or value of the forward pass: lane l of 64 adds features l, l + 64, ... (float64 fused multiply-add), then a butterfly.
 *   Then element i of the gradient = (partial_0[i] + partial_1[i] + ... + partial_{W-1}[i], float32, in this order) / float32(B).
 *   Sum of squares of the 8 488 elements in float64: 34 blocks of 256 consecutive elements, each through a binary tree
 *   (s[i] += s[i + 128], then 64, ... 1), then the 34 block sums in order.  Statistics: per workgroup in sample order, then over w.
 *
 * Optimiser step.  float32, one rounding per operation, no contraction, sqrt and / correctly rounded:
 *   norm = float32(sqrt(sum of squares, float64));   coef = min(1, max_grad_norm / (norm + 1e-6f))   (torch's clip_grad_norm_);
 *   t = steps taken + 1;  on the host in double: bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, then float32: omb1 = 1 - beta1, omb2 = 1 - beta2,
 *   step_size = lr / bc1, bc2s = sqrt(bc2)   (beta1, beta2, lr read as the float32 values passed);
 *   g = grad * coef;   m = beta1 * m + omb1 * g;   v = beta2 * v + omb2 * (g * g);
 *   p = p - step_size * (m / (sqrtf(v) / bc2s + eps))                                      (torch.optim.Adam without amsgrad / decay).
 * Defaults of the Python layer, common PPO practice for this network (Atari-style PPO): clip 0.2, vf_coef 0.5, ent_coef 0.01,
 * lr 2.5e-4, betas (0.9, 0.999), eps 1e-5, max_grad_norm 0.5. */
typedef struct crl_ppo_hyper {
    float clip, vf_coef, ent_coef, lr, beta1, beta2, eps, max_grad_norm;
} crl_ppo_hyper;
typedef struct crl_ppo crl_ppo;
/* Tensors as for crl_policy_create plus the critic of crl_policy_set_critic (host pointers, torch layouts; the critic is required).
 * crl_ppo_set_weights also zeroes both moments and the step count.  Both synchronise the device. */
int crl_ppo_create(int32_t device, const float *conv1_w_host, const float *conv1_b_host, const float *conv2_w_host, const float *conv2_b_host,
                   const float *actor_w_host, const float *actor_b_host, const float *critic_w_host, const float *critic_b_host, crl_ppo **out);
void crl_ppo_destroy(crl_ppo *p);
int crl_ppo_set_weights(crl_ppo *p, const float *conv1_w_host, const float *conv1_b_host, const float *conv2_w_host, const float *conv2_b_host,
                        const float *actor_w_host, const float *actor_b_host, const float *critic_w_host, const float *critic_b_host);
/* The master weights as they stand, into eight host arrays of the torch shapes.  Synchronises the device. */
int crl_ppo_get_weights(crl_ppo *p, float *conv1_w_host, float *conv1_b_host, float *conv2_w_host, float *conv2_b_host, float *actor_w_host,
                        float *actor_b_host, float *critic_w_host, float *critic_b_host);
/* *blob_dev = the master blob on the device (8 488 floats, the layout above), valid until crl_ppo_destroy: what
 * crl_policy_load_weights_dev and crl_pool_load_light_dev take. */
int crl_ppo_weights_dev(crl_ppo *p, const float **blob_dev);
/* The gradient and the statistics of the samples idx_dev[0 .. count) (int64 on the device, flat t * N + e, any order, duplicates
 * allowed, validity the caller's as for crl_rollout_gather), at the learner's current weights; uses hyper's clip, vf_coef, ent_coef.
 * Three launches on `stream`.  Refuses (CRL_EINVAL, before any GPU call) a null argument, count < 1, a rollout that is not finished. */
int crl_ppo_grad(crl_ppo *p, const crl_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper, void *stream);
/* The last gradient: *grad_dev = its device blob (optional; for a caller with an optimiser of its own, overwritten by the next
 * crl_ppo_grad), grad_out_host = a copy of the 8 488 floats (optional; synchronises the device). */
int crl_ppo_get_grad(crl_ppo *p, const float **grad_dev, float *grad_out_host);
/* Clip + Adam on the last gradient, the master blob updated in place: one launch.  Uses hyper's lr, betas, eps, max_grad_norm. */
int crl_ppo_step(crl_ppo *p, const crl_ppo_hyper *hyper, void *stream);
/* out7_host: the five statistics of the last crl_ppo_grad, [5] its gradient's norm (before clipping, float64), [6] the optimiser steps
 * taken.  Synchronises the device (logging, tests). */
int crl_ppo_stats(crl_ppo *p, double *out7_host);
/* crl_policy_load_weights from DEVICE memory: blob_dev (8 488 floats, the layout above, critic included) replaces the weights and the
 * critic of a LightActorCritic policy by one device-to-device copy ordered on `stream`; no host buffer, no synchronisation.  Refuses
 * (CRL_EINVAL, before any GPU call) a null argument and a full-size policy.  crl_pool_load_light_dev: the same into slot `agent` of a
 * league's or an arena's pool (the first 6 884 floats: a slot has no critic); refuses what crl_pool_load_light refuses. */
int crl_policy_load_weights_dev(crl_policy *p, const float *blob_dev, void *stream);
int crl_pool_load_light_dev(crl_league *l, int32_t agent, const float *blob_dev, void *stream);

/* ---- ppo update, full size: the same update for the full-size ActorCritic (utils/network.py:14-50) ----------------
 * The loss, the per-sample closed forms, the statistics and the optimiser step are those of "ppo update", unchanged: temperature 1, an
 * unclipped value loss, every comparison part of the rule, a ReLU's derivative z > 0 ? 1 : 0.  Only the network differs:
 *   x = stack / 255;  z1 = conv1(x) + b1 (4 x 4, stride 2: 16 x 20 x 20),  a1 = max(z1, 0);
 *   z2 = conv2(a1) + b2 (4 x 4, stride 2, padding 2: 32 x 11 x 11),  a2 = max(z2, 0), flattened channel-major to 3872;
 *   z3 = conv3(a2) + b3 (11 x 11 over the whole of a2: the 3872 -> 256 product),  a3 = max(z3, 0);  logits = actor(a3),  v = critic(a3).
 * The three convolutions are float32.  conv1 and conv2 are the served forward pass's arithmetic (conv1 with exact products of the bytes and
 * weight / 255); conv3 is NOT: it adds its products in eleven segments (below), so the logits the learner recomputes agree with those
 * crl_policy_act_rollout served to within float32 rounding, not bit for bit;
 * from the features a3 on the device works in float64 up to dlogits and dv, which are rounded once to float32.
 *
 * Master blob = the blob of a full-size crl_policy, so a push is one device-to-device copy:
 *   w1 [16,4,4,4] | b1 [16] | w2 [32,16,4,4] | b2 [32] | w3 [256,3872] | b3 [256] | wa [3,256] | ba [3] + 1 pad | wc [1,256] | bc [1] + 3 pads
 * = 1 001 784 floats, 1 001 780 of them parameters, torch layouts; pads are zero in the weights, the gradient and both moments and stay so.
 *
 * Summation shape -- a function of B and the learner's scratch_rows S alone, not of the device, the grid or any arrival order; no
 * floating-point atomics; the same idx on the same (B, S) gives the same bits on every run and every learner object.  "Matrix step":
 * one v_mfma_f32_16x16x4_f32, four terms added to a float32 accumulator.
 *   Chunks: samples [0, S), [S, 2 S), ... of idx, in order; row = a sample's place in its chunk.  Every sum below runs over a chunk's
 *   rows as described and carries on from the value the previous chunks left (the accumulator STARTS from it; the first chunk from 0).
 *   z3[c] = (segment_0 + segment_1 + ... + segment_10, float32, in this order) + b3[c]; segment i covers k = 352 i .. 352 i + 351 of a2 and
 *   is one accumulator from 0: 22 slabs of 16 in order, a slab in matrix steps j = 0 .. 3, step j adding the terms k = 16 slab + 4 q + j,
 *   q = 0 .. 3 (the served forward pass runs all 3872 through ONE accumulator; eleven keep the float32 error of a log-probability, and so
 *   of the statistics, near that of its logits).
 *   A logit or v: lane l of 64 adds features l, l + 64, l + 128, l + 192 (float64 fused multiply-add), then a butterfly (32, 16, .. 1).
 *   dz3[c] = (((wa[0][c] dl0) + wa[1][c] dl1) + wa[2][c] dl2) + wc[c] dv, float32 fused multiply-adds after the first product, times (a3[c] > 0).
 *   wa, wc, b3 (column sums of dz3), ba, bc and the statistics, two levels: slice s = the chunk's rows 256 s .. 256 s + 255; a slice's sum
 *   starts from 0 and takes its rows in order (wa, wc: fused multiply-add d[row] * a3[row][c]; the others: additions; the statistics in
 *   float64); then the slices' sums are added in slice order onto the previous chunks' value.  A statistic's mean = its sum / B.
 *   w3[oc][k] (= sum over samples of dz3[oc] a2[k]): one accumulator per element, a matrix step per four consecutive rows in order
 *   (rows past the chunk's end enter as zeros).
 *   dz2[k] = (sum_c dz3[c] w3[c][k]) * (a2[k] > 0): one accumulator from 0, matrix steps g = 0 .. 15, j = 0 .. 3 in this order, step
 *   (g, j) adding the four terms c = 16 g + 4 q + j, q = 0 .. 3.
 *   conv2, conv1: W = min(256, B, S) workgroups; workgroup w takes rows w, w + W, ... of every chunk, in order, into ONE set of
 *   accumulators per launch: w2[oc][ic][tap]: per row 31 matrix steps over the positions 4 s .. 4 s + 3 of 121 (+ 3 zeros), in order;
 *   da1[ic] at a padded position (2 yh + py, 2 xh + px): from 0, 32 matrix steps oc = 0 .. 31, each adding the four taps (py + 2 a, px +
 *   2 b), (a, b) = (0,0), (0,1), (1,0), (1,1), times dz2[oc][yh - a][xh - b];  dz1 = da1 * (a1 > 0);  w1[oc][ic][tap]: per row 100 matrix
 *   steps over the positions 4 s .. 4 s + 3 of 400, B operand = byte / 255 correctly rounded;  b2[oc]: 8 float32 sums, sum i over the
 *   positions i, i + 8, ... of the rows in order, then a butterfly (1, 2, 4) at the launch's end;  b1[oc]: 16 sums over positions i, i + 16,
 *   ..., butterfly (1, 2, 4, 8).  A workgroup's sums of a chunk are ADDED to its partial blob of the chunks before (the first writes it).
 *   Element i of the gradient = (partial_0[i] + ... + partial_{W-1}[i] in this order | the one sum) / float32(B).
 *   Sum of squares in float64: 3 914 blocks of 256 consecutive elements, each through a binary tree (s[i] += s[i + 128], then 64, .. 1);
 *   then 256 sums t = block sums t, t + 256, ... in order, through the same tree.
 *
 * crl_ppo_create_full returns the same crl_ppo type: crl_ppo_grad, _step, _stats, _get_grad (1 001 784 floats), _weights_dev and _destroy
 * work on either kind.  scratch_rows: rows of activation scratch (17.6 KB each), 0 = 16 384, otherwise in [64, 2^20] (a
 * smaller chunk only multiplies launches).  crl_ppo_grad launches eight kernels per chunk and two at the end.  crl_ppo_set_weights / _get_weights refuse a full-size learner and the _full variants a light one
 * (CRL_EINVAL, before any GPU call).  Tensors: host pointers, torch layouts (conv3 [256,32,11,11]); the critic is required. */
int crl_ppo_create_full(int32_t device, int64_t scratch_rows, const float *conv1_w_host, const float *conv1_b_host, const float *conv2_w_host,
                        const float *conv2_b_host, const float *conv3_w_host, const float *conv3_b_host, const float *actor_w_host,
                        const float *actor_b_host, const float *critic_w_host, const float *critic_b_host, crl_ppo **out);
int crl_ppo_set_weights_full(crl_ppo *p, const float *conv1_w_host, const float *conv1_b_host, const float *conv2_w_host, const float *conv2_b_host,
                             const float *conv3_w_host, const float *conv3_b_host, const float *actor_w_host, const float *actor_b_host,
                             const float *critic_w_host, const float *critic_b_host);
int crl_ppo_get_weights_full(crl_ppo *p, float *conv1_w_host, float *conv1_b_host, float *conv2_w_host, float *conv2_b_host, float *conv3_w_host,
                             float *conv3_b_host, float *actor_w_host, float *actor_b_host, float *critic_w_host, float *critic_b_host);
/* The full-size learner's blob (crl_ppo_weights_dev: 1 001 784 floats, critic included) into a full-size policy, or its first 1 001 524
 * floats into full-size slot `agent` of a pool (a slot has no critic): one device-to-device copy ordered on `stream`.  Refuse
 * (CRL_EINVAL, before any GPU call) a null argument and a LightActorCritic policy / what crl_pool_load_full refuses.
 * crl_policy_load_weights_dev keeps refusing a full-size policy: its blob is the light learner's. */
int crl_policy_load_full_dev(crl_policy *p, const float *blob_dev, void *stream);
int crl_pool_load_full_dev(crl_league *l, int32_t agent, const float *blob_dev, void *stream);

/* ---- ppo update, teacher targets: imitation and KL-to-teacher on either learner ----------------
 * Extends "ppo update" (and "ppo update, full size"); nothing in those sections changes.  One term is added to d loss / d logits in the
 * heads; everything behind the heads -- backward passes, summation shapes, reduce, optimiser step, push, resume -- is untouched.  Serves
 * distilling one network into another (teacher logits), cloning a rule (labels, e.g. crl_rule_labels) and PPO regularised towards a teacher.
 *
 * Target distribution q of sample b, from row s = idx[b] (the flat t * N + e index; never row b) of one of two device arrays:
 *   logits  float32 [T * N][3], at temperature tau, in float64:  u_k = (double) l_k / (double) tau,  m = max u,  e_k = exp(u_k - m),
 *           S = (e0 + e1) + e2,  q_k = e_k / S,  logq_k = (u_k - m) - log S;
 *   labels  int32 [T * N]: a value in 0..2 gives the one-hot q (a term with q_k = 0 counts as 0); any other value means the sample has
 *           no teacher: its teacher term and its teacher statistics are 0.
 * Learner side: logp_k, p_k exactly as "ppo update" forms them (the learner's temperature stays fixed at 1), and
 *   ce = -((q0 logp0 + q1 logp1) + q2 logp2),   Hq = -((q0 logq0 + q1 logq1) + q2 logq2),   kl = ce - Hq   (= KL(q || p)).
 * Loss, per sample:   loss_b = policy_term * policy + coef * ce + vf * value - ent * entropy,
 *   policy_term in {0, 1}: at 0 the rule sets d policy / d logp = 0 -- pure imitation; the stored advantage and old log-prob then play
 *   no part in the gradient (they still enter the five statistics);  coef >= 0;
 *   value = 0.5 (target - v)^2 with target = the stored return, or row s of an optional float32 array value_targets [T * N] (a teacher's critic).
 * Closed form, float64, rounded once to float32:   d loss_b / d logit_k = (the expression of "ppo update") + coef (p_k - q_k), the
 * teacher term added last;  d loss_b / d v = vf (v - target).  With coef = 0, policy_term = 1 and no value targets the gradient
 * therefore equals crl_ppo_grad's as numbers.
 * Statistics: the five of "ppo update" as always, and four more, float64 sums over the samples / B: ce, kl, agree = 1[argmax p ==
 * argmax q] (the lowest index among equals on both sides; taken over the logits and over u), labelled = the share of samples with a
 * teacher term.  They use the summation shape the five have on each learner: per workgroup then over workgroups (light); rows, then
 * slices, then chunks (full size).
 * The kernels: the teacher instantiations of the gradient kernel (light) and of the heads, head-slice, head-sum and final kernels (full
 * size); the plain instantiations are what crl_ppo_grad launches, unchanged.  The same launches, no floating-point atomics, the same call
 * gives the same bits on every run, nothing synchronises, all work is ordered on the caller's stream. */
typedef struct crl_ppo_teacher {
    const float *logits_dev;          /* [rows][3] or null */
    const int32_t *labels_dev;        /* [rows] or null; exactly one of the two */
    const float *value_targets_dev;   /* [rows] or null = the stored returns */
    int64_t rows;                     /* must equal T * N of the rollout */
    float temperature, coef;
    int32_t policy_term;
} crl_ppo_teacher;
/* crl_ppo_grad with a teacher, on either kind of learner; crl_ppo_step, _stats, _get_grad and _weights_dev work behind it as behind
 * crl_ppo_grad.  The teacher's arrays are the caller's and must stay valid until the launches have run.  Refuses (CRL_EINVAL, before any
 * GPU call, the learner as it was): everything crl_ppo_grad refuses; a null teacher; both of logits and labels, or neither; rows != T * N;
 * a temperature that is not finite and > 0; a coef that is not finite and >= 0; policy_term outside {0, 1}; a teacher array that is
 * not 4-byte aligned. */
int crl_ppo_grad_teacher(crl_ppo *p, const crl_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper,
                         const crl_ppo_teacher *teacher, void *stream);
/* out4_host: ce, kl, agree, labelled of the last crl_ppo_grad_teacher.  Synchronises the device, like crl_ppo_stats.  Refuses
 * (CRL_EINVAL) when the learner's last gradient was a plain crl_ppo_grad's, or when it has none. */
int crl_ppo_teacher_stats(crl_ppo *p, double *out4_host);

/* ---- checkpoint / resume: what a training loop needs to stop and go on, bit for bit ----------------
 * The reference's trainers checkpoint the model's state_dict and the optimiser's (torch.save); a loop that never leaves the device
 * also has to carry what lives on the device only.  Per object, the state is:
 *
 *   crl_ctx (Pong, CarRacing)  crl_get_state / crl_set_state, crl_car_get_state / _set_state (above).
 *   crl_ledger, crl_arena      counters, running episodes, draw counters, weights, seed (their get / set calls above).
 *   crl_policy                 the weight blob AS THE DEVICE HOLDS IT (after crl_policy_load_weights_dev / _load_full_dev the host has
 *                              no copy), whether it carries a critic, the frame ring (crl_policy_get_stack), the play style
 *                              (temperature, epsilon, seed, env_id_base) and its call counter, the n of "sampled actions".
 *   crl_league (the pool)      per CNN slot the weight blob as the device holds it, the seed, the act-call counter (the n of RANDOM's
 *                              and of every sampled or explored action), the per-env opponent draw counters, the play styles
 *                              (crl_sampling_get_agent), the assignment (crl_league_get_assignment), the rings (crl_league_get_stack).
 *   crl_rollout                where the rollout stands (fresh / in progress / finished, steps recorded, steps with an outcome, whether
 *                              the finish normalised), the three planes in front of step 0 with their depth, every recorded step's
 *                              plane, reset flag, depth, action, log-prob and value, every outcome's reward and done, and after the
 *                              finish returns, advantages and the two float64 statistics.
 *   crl_ppo                    the master blob, Adam's two moments in the blob's layout (pads zero), the optimiser steps taken and,
 *                              full size, scratch_rows (part of the summation shape).  The last gradient and its statistics are NOT
 *                              state: after crl_ppo_set_state the learner has no gradient until the next crl_ppo_grad.
 *
 * The getters that fill HOST memory copy on `stream` and wait for that copy: they are ordered behind the work enqueued on `stream`
 * (a crl_policy_load_weights_dev, a crl_ppo_step) and synchronise with it.  The setters are ordered on `stream` likewise and return
 * when their copies are done, so the caller's buffers are free again.  Nothing here is for the hot loop, and no act / record / grad /
 * step launch changes.  All refuse (CRL_EINVAL, before any GPU call) a null object and what is said below. */
/* The policy's blob, critic tail included: `blob_floats` must be 8 488 (LightActorCritic: conv1 | b1 | conv2 | b2 | actor | ba + 1 pad |
 * critic | bc + 3 pads, torch layouts) or 1 001 784 (full size: conv1 | b1 | conv2 | b2 | conv3 | b3 | actor | ba + 1 pad | critic |
 * bc + 3 pads), the policy's own.  has_critic_out (optional): 1 if a critic was ever set (the tail is zero otherwise). */
int crl_policy_get_blob(crl_policy *p, float *blob_out_host, int64_t blob_floats, int32_t *has_critic_out, void *stream);
/* The play style as crl_policy_set_sampling took it, and the call counter: crl_policy_act / _act_rollout calls since create or the last
 * crl_policy_set_sampling.  Every out pointer is optional.  Host values, no GPU work. */
int crl_policy_get_sampling(crl_policy *p, float *temperature, float *epsilon, uint64_t *seed, int64_t *env_id_base, uint32_t *calls);
/* crl_policy_set_sampling that continues at call `calls` instead of 0: the next act call draws with n = calls. */
int crl_policy_resume_sampling(crl_policy *p, float temperature, float epsilon, uint64_t seed, int64_t env_id_base, uint32_t calls);
/* Slot `agent`'s blob (a slot has no critic): `blob_floats` must be 6 884 (CRL_LEAGUE_LIGHT) or 1 001 524 (CRL_POOL_KIND_FULL), the
 * slot's own; a built-in agent has none and is refused. */
int crl_pool_get_blob(crl_league *l, int32_t agent, float *blob_out_host, int64_t blob_floats, void *stream);
/* The pool's counters.  seed, env_id_base, act_calls (the crl_league_act calls since create / crl_league_seed): optional host values;
 * draw_ctr_out_dev: optional uint32 [num_envs] on the device, a copy enqueued on `stream` (no synchronisation). */
int crl_pool_get_counters(crl_league *l, uint64_t *seed, int64_t *env_id_base, uint32_t *act_calls, uint32_t *draw_ctr_out_dev, void *stream);
/* ... and their setter (the seed is crl_league_seed's, which zeroes both counters: call it first).  draw_ctr_dev: uint32 [num_envs] on
 * the device or NULL (the draw counters stay); the copy is enqueued on `stream`, the buffer is the caller's until it has run. */
int crl_pool_set_counters(crl_league *l, uint32_t act_calls, const uint32_t *draw_ctr_dev, void *stream);
/* Where the rollout stands: out4_host = {0 fresh / 1 in progress / 2 finished, steps recorded, steps with an outcome, 1 if the finish
 * normalised}.  Host values, no GPU work. */
int crl_rollout_get_info(crl_rollout *r, int32_t *out4_host);
/* Copies of the storage's arrays into DEVICE buffers of the caller, enqueued on `stream` (no synchronisation); every pointer is
 * optional.  planes_out_dev: u8 [rows][N][42][42], plane rows row0 .. row0 + rows - 1 of the T + 3 the storage holds (rows 0 .. 2 are
 * the planes in front of step 0, row t + 3 is step t's), without the padding; front_depth_out_dev: u8 [N], the depth those three
 * planes are carried at.  The per-step arrays hold steps [0, steps): reset, depth, done u8 [steps][N], actions int32, logp, values,
 * rewards float32.  returns / adv: float32 [T][N], stats: float64 [2] (mean, std); what they hold before a finish is unspecified.
 * Refuses rows outside [0, T + 3] and steps outside [0, T]. */
int crl_rollout_get_state(crl_rollout *r, int64_t row0, int64_t rows, uint8_t *planes_out_dev, uint8_t *front_depth_out_dev, int64_t steps,
                          uint8_t *reset_out_dev, uint8_t *depth_out_dev, int32_t *actions_out_dev, float *logp_out_dev, float *values_out_dev,
                          float *rewards_out_dev, uint8_t *done_out_dev, float *returns_out_dev, float *adv_out_dev, double *stats_out_dev,
                          void *stream);
/* The reverse: info4_host as crl_rollout_get_info gives it, looked at before anything is written (state in [0, 2]; outcomes <= recorded
 * <= T; fresh: both 0; finished: both T), the arrays as above (NULL: that array stays).  The copies are enqueued on `stream`; the
 * buffers are the caller's until they have run. */
int crl_rollout_set_state(crl_rollout *r, const int32_t *info4_host, int64_t row0, int64_t rows, const uint8_t *planes_dev,
                          const uint8_t *front_depth_dev, int64_t steps, const uint8_t *reset_dev, const uint8_t *depth_dev,
                          const int32_t *actions_dev, const float *logp_dev, const float *values_dev, const float *rewards_dev,
                          const uint8_t *done_dev, const float *returns_dev, const float *adv_dev, const double *stats_dev, void *stream);
/* The learner's master blob and Adam's two moments, each `blob_floats` floats in the blob's layout (8 488 or 1 001 784, the learner's
 * own; each pointer optional), the optimiser steps taken and scratch_rows (0 for the light learner). */
int crl_ppo_get_state(crl_ppo *p, float *blob_out_host, float *m_out_host, float *v_out_host, int64_t blob_floats, int64_t *steps_out,
                      int64_t *scratch_rows_out, void *stream);
/* Weights, moments and step count together (crl_ppo_set_weights* keep zeroing the moments): all three blobs are required, steps >= 0.
 * The learner then has no gradient: crl_ppo_step / _stats / _get_grad refuse until the next crl_ppo_grad. */
int crl_ppo_set_state(crl_ppo *p, const float *blob_host, const float *m_host, const float *v_host, int64_t blob_floats, int64_t steps,
                      void *stream);

/* ---- car drivers: built-in CarRacing agents served from the env's own device state --------------
 * Stands in for the opponent_policy of make_competitive_car_racing (car_racing/make_competitive_car_racing.py:10-58), for which the
 * reference ships nothing, and is CarRacing's counterpart of Pong's RANDOM and RULE_BASED (pong/builtin_policies.py:44-58): RULE_BASED
 * reads the env's state, as the cheat code does.  An object beside a CarRacing context (as the ledger is beside the league): it READS
 * the context's committed state and writes the caller's action tensor, nothing else.  One launch per crl_car_driver_act on the
 * caller's stream serves every car of every env; nothing synchronises with the host.
 *
 * Styles and assignment.  Up to CRL_CAR_DRIVER_SLOTS styles: kind (enum crl_car_driver_kind), target_speed (float32, world units per
 * second), lookahead (tiles, 0..CRL_CAR_DRIVER_MAX_LOOKAHEAD), steer_gain (float32), epsilon (float32 in [0, 1]).  Slot 0 is preset
 * to RANDOM, slot 1 to RULE_BASED with CRL_CAR_DRIVER_DEFAULT_* (epsilon 0); the other slots are empty until set.  The assignment is
 * an int32 per (env, car), [N][players]: the car's style slot; a value outside [0, CRL_CAR_DRIVER_SLOTS) -- -1 by convention, the
 * state after create -- or an empty slot leaves the car's two floats of the action tensor as they are.
 *
 * The rule (rules.car_driver_reference restates it in numpy, bit for bit).  Everything is float32 with ONE rounding per operation: no
 * contraction, no fast-math intrinsics, sqrt and / correctly rounded; a + b + c is never written, every sum below has two terms.
 * Inputs of car c of env i: its hull body's cx, cy, vx, vy; the centres (wx_k, wy_k) of its wheel bodies k = 0..3 (WHEELPOS order,
 * car_racing/car_dynamics.py:23-26: 0, 1 front, 2, 3 rear); its done flag; the env's tile count n and tile boxes (x0, y0, x1, y1)_t,
 * t < n (the minimum and maximum of the tile polygon's five float32 vertices).  Output (steer, gas): the env's two-component action
 * (process_action, car_racing_multi_players.py:528-540): steer > 0 turns right (the env applies steer(-a[0]), :554), gas > 0
 * accelerates, gas < 0 brakes.
 *   0. done != 0 or n <= 0: (0, 0).  Nothing below is evaluated.
 *   1. draw: ONE call x = Philox4x32-10(counter = (gid & 0xFFFFFFFF, gid >> 32, call, CRL_CAR_DRIVER_DOMAIN + c), key = (seed &
 *      0xFFFFFFFF, seed >> 32)) -- the generator of "league draws"; gid = env_id_base + i, the env's GLOBAL id (the context's
 *      env_id_base), call = the number of crl_car_driver_act calls since create / crl_car_driver_set_counters (0 for the first; it
 *      moves for every car, assigned or not) -- gives x0..x3.  unit(x) = float32(int32(x >> 8) - 8388608) * 2^-23, in [-1, 1), exact.
 *      RANDOM: (unit(x0), unit(x1)).  RULE_BASED: with eps_q = min(floor(epsilon * 2^32), 0xFFFFFFFF) (in double from the float32
 *      epsilon, as "sampled actions"), if x2 < eps_q the action is RANDOM's; epsilon has no effect on RANDOM.
 *   2. nearest tile: tx_t = (x0_t + x1_t) * 0.5, ty_t = (y0_t + y1_t) * 0.5; dx = tx_t - cx, dy = ty_t - cy;
 *      d_t = (dx * dx) + (dy * dy), a NaN d_t counts as +inf; nearest = the t < n with the smallest d_t, the LOWEST t among equals.
 *   3. target: g = (nearest + lookahead) mod n;  ax = tx_g - cx, ay = ty_g - cy.
 *   4. heading, without trigonometry: hx = (wx_0 + wx_1) * 0.5 - (wx_2 + wx_3) * 0.5, hy likewise: rear axle's midpoint to front's.
 *      cr = (hx * ay) - (hy * ax);  dt = (hx * ax) + (hy * ay);  den = sqrt((hx * hx) + (hy * hy)) * sqrt((ax * ax) + (ay * ay)).
 *      If den > 0: sn = cr / den, cs = dt / den; otherwise (zero, or NaN) sn = 0, cs = 1.
 *      e = sn if cs >= 0; otherwise (the target lies behind) 1 if sn > 0, -1 if sn < 0, else 0.
 *   5. steer = clamp(-(steer_gain * e)).
 *   6. v = sqrt((vx * vx) + (vy * vy));  want = target_speed * (1 - CRL_CAR_DRIVER_CURVE_SLOW * |e|);
 *      gas = clamp((want - v) * CRL_CAR_DRIVER_GAS_GAIN).
 *   clamp(x) = -1 if x < -1, 1 if x > 1, else x (a NaN passes).
 * A draw depends on (seed, global env id, car, call) alone and the rest on the env's state: shards of a batch act as the whole batch.
 * The default style's constants were tuned closed loop on the CPU checker (docs/LAB_NOTES_car_drivers.md). */
#define CRL_CAR_DRIVER_SLOTS 16
#define CRL_CAR_DRIVER_MAX_LOOKAHEAD 64
#define CRL_CAR_DRIVER_DOMAIN 0x43524430u /* "CRD0"; car 1 draws under "CRD1" */
#define CRL_CAR_DRIVER_GAS_GAIN 0.1f
#define CRL_CAR_DRIVER_CURVE_SLOW 0.5f
#define CRL_CAR_DRIVER_DEFAULT_TARGET_SPEED 45.0f
#define CRL_CAR_DRIVER_DEFAULT_LOOKAHEAD 4
#define CRL_CAR_DRIVER_DEFAULT_STEER_GAIN 1.5f
enum crl_car_driver_kind { CRL_CAR_DRIVER_RANDOM = 0, CRL_CAR_DRIVER_RULE_BASED = 1 };
typedef struct crl_car_driver crl_car_driver;
/* Drivers for the envs of CarRacing context `ctx`, which must outlive them; seed = the key of the draws.  Refuses (CRL_EINVAL, before
 * any GPU call) a null argument and a Pong context. */
int crl_car_driver_create(crl_ctx *ctx, uint64_t seed, crl_car_driver **out);
void crl_car_driver_destroy(crl_car_driver *d);
/* Style slot `slot`, from the next crl_car_driver_act on; host values, no GPU call.  Refuses (CRL_EINVAL; the values are looked at
 * first, then the handle) a slot outside [0, CRL_CAR_DRIVER_SLOTS), a kind outside the enum, a non-finite or negative target_speed or
 * steer_gain, a lookahead outside [0, CRL_CAR_DRIVER_MAX_LOOKAHEAD] and an epsilon outside [0, 1].  _get_style: kind -1 = empty. */
int crl_car_driver_set_style(crl_car_driver *d, int32_t slot, int32_t kind, float target_speed, int32_t lookahead, float steer_gain,
                             float epsilon);
int crl_car_driver_get_style(crl_car_driver *d, int32_t slot, int32_t *kind, float *target_speed, int32_t *lookahead, float *steer_gain,
                             float *epsilon);
/* ids_dev int32 [N][players] on the device, copied (device to device, on `stream`) into the driver's own array. */
int crl_car_driver_set_assignment(crl_car_driver *d, const int32_t *ids_dev, void *stream);
int crl_car_driver_get_assignment(crl_car_driver *d, int32_t *ids_out_dev, void *stream);
/* opponent_policy(obs) for every assigned car: actions_dev float32 [N][players][2], the layout crl_step takes.  Enqueued on `stream`
 * behind a crl_step / crl_reset of the context on the same stream it sees the state that call committed, the auto-reset of finished
 * envs included -- the observation the reference's wrapper hands its opponent (make_competitive_car_racing.py:24-33). */
int crl_car_driver_act(crl_car_driver *d, float *actions_dev, void *stream);
/* Resume: the key and the act-call counter (host values; calls in [0, 2^32)). */
int crl_car_driver_get_counters(crl_car_driver *d, uint64_t *seed, int64_t *calls);
int crl_car_driver_set_counters(crl_car_driver *d, uint64_t seed, int64_t calls);

/* ---- car policy: a state observation and the reference's MLP, served per env and per car ---------
 * What "serve a learner" is for Pong, for CarRacing: the reference's MLP(input_size, output_size) (utils/network.py:59-70: fc1 -> 100,
 * ReLU, policy, value) on a per-car STATE observation computed from the context's committed state, served per env and per car from
 * CRL_CAR_POLICY_SLOTS weight sets, with Gaussian actions, values and log-probabilities for a trainer.  An object beside a CarRacing
 * context, as the car drivers are: it READS the state and writes the caller's tensors.  One launch per crl_car_policy_act /
 * _observe on the caller's stream; nothing synchronises with the host.  rules.car_obs_reference, rules.car_mlp_reference and
 * rules.car_policy_reference (with car_policy_noise and car_policy_sample) restate this section in numpy.
 *
 * As in "car drivers": everything is float32 with ONE rounding per operation, no contraction, no fast-math intrinsic, / and sqrt
 * correctly rounded; every sum has two terms or the shape written here.
 * Inputs of car c of env i: its hull body (cx, cy, a, vx, vy, w); its wheel bodies k = 0..3 (wx_k, wy_k, wa_k; 0, 1 front, 2, 3 rear);
 * its done flag and visited_count; touch_k = wheel k touches at least one tile; the env's tile count n and tile boxes; for
 * players == 2 the other car's hull (ocx, ocy, ovx, ovy) and done flag.
 *
 * Observation: CRL_CAR_OBS_FEATURES = 21 float32.  done != 0 or n <= 0: all 21 are +0 and nothing below is evaluated.  Otherwise
 *   frame: (hx, hy) exactly as rule 4 of "car drivers";  len = sqrt((hx * hx) + (hy * hy));  forward f = (hx / len, hy / len) if
 *     len > 0, otherwise (zero, or NaN) (1, 0);  left l = (-f.y, f.x);  car(v) = ((v.x * f.x) + (v.y * f.y), (v.x * l.x) + (v.y * l.y)).
 *   [0], [1]   car((vx, vy)) * CRL_CAR_OBS_SPEED_SCALE, componentwise
 *   [2]        w * 2^-2
 *   [3]        (wa_0 - a) * 2
 *   [4]        (the number of k with touch_k, as float32) * 0.25
 *   [5]        float32(visited_count) / float32(n)
 *   [6 + 2 m], [7 + 2 m], m = 0..4: with nearest = rule 2 of "car drivers" and o_m = (0, 2, 4, 8, 16)[m]: g = (nearest + o_m) mod n,
 *              car((tx_g - cx, ty_g - cy)) * CRL_CAR_OBS_DIST_SCALE  (tx, ty: the box centres of rule 2)
 *   [16], [17] car((ocx - cx, ocy - cy)) * CRL_CAR_OBS_DIST_SCALE
 *   [18], [19] car((ovx - vx, ovy - vy)) * CRL_CAR_OBS_SPEED_SCALE
 *   [20]       1 if the other car is not done, else 0
 *   players == 1: [16..20] are +0.
 * Every scale is a power of two: the scaling is exact.
 *
 * Network.  Weights of one slot: fc1_w (100, 21), fc1_b (100), policy_w (2, 100), policy_b (2), value_w (1, 100), value_b (1) -- the
 * reference's MLP(21, 2) -- and log_std (2), which the reference's class lacks (0 where a checkpoint has none).  With x the observation:
 *   hidden_j = relu(a_j), j < 100:  a_j starts as fc1_b[j]; then for k = 0, 1, .., 20 IN THIS ORDER a_j = a_j + (fc1_w[j][k] * x[k]);
 *     relu(a) = a if a > 0, else +0.
 *   each output o of (mean_0, mean_1, value), with row r_o = policy_w[0], policy_w[1], value_w[0] and bias policy_b[0], policy_b[1],
 *     value_b[0]: the 64 partial sums p_L = hidden_L * r_o[L] for L < 64, and for L < 36 p_L = p_L + (hidden_{L+64} * r_o[L + 64]);
 *     then the butterfly: for m = 32, 16, 8, 4, 2, 1 IN THIS ORDER every p_L = p_L + p_{L xor m} (all 64 at once; float addition
 *     commutes, so all 64 hold the same bits);  o = p_0 + bias.
 *   std_d = float32(exp(float64(log_std_d))), computed by whoever packs the blob, on the host: the kernel evaluates no exp.
 * The blob of one slot, CRL_CAR_POLICY_BLOB_FLOATS float32: fc1_w TRANSPOSED [21][100] at 0 (a lane reads its hidden unit's weight
 * of input k beside its neighbours'), fc1_b at 2100, policy_w [2][100] at 2200, value_w [100] at 2400, then at 2500: policy_b[0],
 * policy_b[1], value_b[0], log_std_0, log_std_1, std_0, std_1, one pad.  rules.car_policy_pack / car_policy_unpack.
 *
 * Action.  The env clips actions itself (process_action, car_racing_multi_players.py:528-540): u is written unclipped.
 *   done != 0 or n <= 0: u = (0, 0), value 0, log_prob 0, z = (0, 0).
 *   deterministic slot: u = mean, log_prob = 0, z = (0, 0).
 *   sampling slot: ONE call x = Philox4x32-10(counter = (gid & 0xFFFFFFFF, gid >> 32, call, CRL_CAR_POLICY_DOMAIN + c), key = (seed &
 *     0xFFFFFFFF, seed >> 32)), gid and call as rule 1 of "car drivers" (call counts crl_car_policy_act calls; _observe does not move
 *     it).  Component d = 0, 1 takes (x_{2d}, x_{2d+1}):
 *       u1 = float32((x_{2d} >> 8) + 1) * 2^-24, in (0, 1], exact;   u2 = float32(x_{2d+1} >> 8) * 2^-24, in [0, 1), exact;
 *       L = log(u1): a float32 natural logarithm with an error of at most 1 ulp (the kernel: the device library's logf; rules: the
 *         float64 logarithm rounded to float32);   r = sqrt(-2 * L)  (-2 * L is exact);
 *       t = CRL_CAR_POLICY_TWO_PI * u2;   cs = the cosine of include/crl_rot.h's crl_sincosf(t) (correctly rounded);   z_d = r * cs.
 *     u_d = mean_d + (std_d * z_d);
 *     log_prob = ((((-0.5 * z_0) * z_0) - log_std_0) + (((-0.5 * z_1) * z_1) - log_std_1)) - CRL_CAR_POLICY_LN_2PI.
 *   Against Z_d = sqrt(-2 ln u1) cos(2 pi u2) in exact arithmetic, with R = sqrt(-2 ln u1) <= 5.77: 1 ulp of L and the square root's
 *   rounding move r by at most R * 2^-23; the rounded 2 pi and the product move t by at most 2 pi * 2^-23, the cosine's rounding adds
 *   2^-25; the last product adds R * 2^-24:  |z_d - Z_d| <= R * 2^-23 * (2 pi + 2)  (the 0.25 beyond 2 pi + 1.75 covers the
 *   second-order terms).  Only z differs between evaluations of L; given z, u and log_prob follow bit for bit.
 * A draw depends on (seed, global env id, car, call) alone and the rest on the env's state: shards act as the whole batch. */
#define CRL_CAR_OBS_FEATURES 21
#define CRL_CAR_OBS_SPEED_SCALE 0x1p-6f
#define CRL_CAR_OBS_DIST_SCALE 0x1p-5f
#define CRL_CAR_POLICY_SLOTS 8
#define CRL_CAR_POLICY_HIDDEN 100
#define CRL_CAR_POLICY_BLOB_FLOATS 2508
#define CRL_CAR_POLICY_DOMAIN 0x43525030u /* "CRP0"; car 1 draws under "CRP1" */
#define CRL_CAR_POLICY_TWO_PI 0x1.921fb6p+2f
#define CRL_CAR_POLICY_LN_2PI 0x1.d67f1cp+0f /* float32(ln(2 pi)) */
typedef struct crl_car_policy crl_car_policy;
/* A policy server for the envs of CarRacing context `ctx`, which must outlive it; seed = the key of the draws.  Every slot is empty
 * and every car unassigned (-1).  Refuses (CRL_EINVAL, before any GPU call) a null argument and a Pong context. */
int crl_car_policy_create(crl_ctx *ctx, uint64_t seed, crl_car_policy **out);
void crl_car_policy_destroy(crl_car_policy *p);
/* The blob of slot `slot` (host or device memory, CRL_CAR_POLICY_BLOB_FLOATS floats), copied on `stream`: no device synchronisation,
 * and launches enqueued on `stream` after this call see the new weights.  deterministic: 0 = sampling, 1 = u = mean; it holds for
 * the launches enqueued after the call.  The argument checks are those of crl_car_driver_*: the values first (slot outside [0,
 * CRL_CAR_POLICY_SLOTS), deterministic outside {0, 1}), then the handle and the pointer; CRL_EINVAL before any GPU call. */
int crl_car_policy_set_weights(crl_car_policy *p, int32_t slot, const float *blob_host_or_dev, int32_t deterministic, void *stream);
/* What the device holds: the blob (to host or device memory, on `stream`; the caller synchronises `stream` before reading a host
 * buffer; optional) and the flag (optional).  An empty slot is refused. */
int crl_car_policy_get_weights(crl_car_policy *p, int32_t slot, float *blob_out_host_or_dev, int32_t *deterministic_out, void *stream);
/* The flag of a loaded slot alone (host value, no GPU call). */
int crl_car_policy_set_sampling(crl_car_policy *p, int32_t slot, int32_t deterministic);
/* int32 [N][players] on the device: the car's slot; a value outside [0, CRL_CAR_POLICY_SLOTS) -- -1 by convention -- or an empty slot
 * means nobody: the car's floats of the action tensor stay as they are. */
int crl_car_policy_set_assignment(crl_car_policy *p, const int32_t *ids_dev, void *stream);
int crl_car_policy_get_assignment(crl_car_policy *p, int32_t *ids_out_dev, void *stream);
/* One launch: u into actions_dev float32 [N][players][2] for the served cars (the others are left as written); optionally (null =
 * not wanted) values [N][players], log_probs [N][players], noise z [N][players][2] -- each 0 for a car nobody serves -- and the
 * observation [N][players][21] of EVERY car.  Sees the state the last crl_step / crl_reset on `stream` committed. */
int crl_car_policy_act(crl_car_policy *p, float *actions_dev, float *values_dev, float *log_probs_dev, float *noise_dev, float *obs_dev,
                       void *stream);
/* The observation [N][players][21] of every car; no network runs and the call counter does not move. */
int crl_car_policy_observe(crl_car_policy *p, float *obs_dev, void *stream);
/* Resume: the key and the act-call counter (host values; calls in [0, 2^32)). */
int crl_car_policy_get_counters(crl_car_policy *p, uint64_t *seed, int64_t *calls);
int crl_car_policy_set_counters(crl_car_policy *p, uint64_t seed, int64_t calls);

/* ---- car rollout storage: T steps of a CarRacing learner's rollout on the device, GAE, minibatch gather ----------
 * What "rollout storage" is for Pong, for the car policy: an object beside a CarRacing context, as crl_car_policy is.  It stores what
 * crl_car_policy_act wrote for the chosen cars and READS the context's committed per-car done flags and tile counts, and crl_car_info's
 * done_car, itself.  The whole learner loop stays on the device: act -> record -> crl_step (no frame drawn) -> outcome -> finish ->
 * crl_car_ppo_grad / _step -> crl_car_policy_set_weights; no call below synchronises with the host but _stats and _get/_set_state's
 * callers.  rules.gae_reference restates the GAE rule.
 *
 * Rows.  cars_mask: bit c = car c is stored (1, 2 or 3).  C = the number of stored cars, rows R = N * C, row = e * C + j (j-th stored
 * car of env e), flat sample index = t * R + row; T * R < 2^31.
 * Layout: ONE SAMPLE = ONE ALIGNED 128-BYTE LINE of 32 words: obs[21], u[2], log-prob, value, reward, return, advantage, a flags word
 * (bit 0 live, bit 1 done), three words of padding.  The update fetches samples by random index: a gradient lane touches exactly one
 * line per sample (128 bytes moved per sample, all of them used but 12); GAE's strided walk over t costs T * R lines once per rollout.
 *
 * live(t, row) = the car's assignment in `policy` on the device equals `slot`, and the car's done flag is 0, and the env's tile count
 * is > 0, all as crl_car_policy_act of step t saw them: the conditions under which that call served a real sample.  A dead sample (an
 * all-zero observation, log-prob 0) is stored but is not training material: it takes no part in the statistics or in the gradient.
 * done(t, row) = done[e] != 0 || done_car[e][c] != 0 after the step: the second term covers CRL_CAR_DONE_CAR0, where a finished car 1
 * stays frozen in the world while car 0 drives on.
 * GAE: the rule of "rollout storage", unchanged, one lane per row, with done(t, row) and last_values[e][c].
 * Statistics (normalize != 0): mean and unbiased deviation of the LIVE samples' advantages in float64, in the summation shape of
 * "rollout storage" over the flat index, a dead sample contributing 0; divisors L and L - 1 with L the live count; the mean is 0 where
 * L = 0 and the deviation 0 where L < 2.  A gathered advantage is (adv - float32(mean)) / (float32(std) + 1e-5f).
 * State machine: as crl_rollout_*: record(t) needs t == the steps recorded so far, outcome(t) a record of t and t == the outcomes so
 * far, finish all T outcomes, gather / the gradient a finish; begin rewinds (there is no frame history to carry).  Every out-of-order
 * call is refused with CRL_EINVAL before any GPU call. */
typedef struct crl_car_rollout crl_car_rollout;
/* A storage of num_steps steps for the cars of cars_mask of CarRacing context `ctx`, which must outlive it, on the current device.
 * Refuses a Pong context, a mask outside 1..3 or naming a car the context lacks, num_steps < 1, T * R >= 2^31. */
int crl_car_rollout_create(crl_ctx *ctx, int64_t num_steps, int32_t cars_mask, crl_car_rollout **out);
void crl_car_rollout_destroy(crl_car_rollout *r);
int crl_car_rollout_begin(crl_car_rollout *r);
/* Step t: the full contiguous tensors the crl_car_policy_act call of this step just wrote on `stream` -- obs [N][players][21], actions
 * [N][players][2], values and log_probs [N][players] -- of which the stored cars' columns are kept, and `live` for network `slot` of
 * `policy` (a policy of the SAME context; its assignment is copied on `stream`).  A deterministic or empty slot is refused. */
int crl_car_rollout_record(crl_car_rollout *r, int64_t t, crl_car_policy *policy, int32_t slot, const float *obs_dev, const float *actions_dev,
                           const float *values_dev, const float *log_probs_dev, void *stream);
/* What crl_step answered to step t: rewards float32 [N][players] and done u8 [N] as the step wrote them. */
int crl_car_rollout_outcome(crl_car_rollout *r, int64_t t, const float *rewards_dev, const uint8_t *done_dev, void *stream);
/* last_values float32 [N][players] (the values of the act call that opens the next rollout) or null = zeros. */
int crl_car_rollout_finish(crl_car_rollout *r, const float *last_values_dev, double gamma, double lam, int32_t normalize, void *stream);
/* The samples idx_dev (int64 flat indices, any order, duplicates allowed; a bad index only READS inside the storage): obs [B][21],
 * actions [B][2], old log-probs, values, returns, advantages (normalised if the finish was) float32 [B], live u8 [B]; each optional. */
int crl_car_rollout_gather(crl_car_rollout *r, const int64_t *idx_dev, int64_t count, float *obs_out_dev, float *actions_out_dev, float *logp_out_dev,
                           float *values_out_dev, float *returns_out_dev, float *adv_out_dev, uint8_t *live_out_dev, void *stream);
/* mean, std, live count L after a normalising finish (synchronises the device). */
int crl_car_rollout_stats(crl_car_rollout *r, double *out3_host);
/* Resume.  out8: state (0 fresh, 1 active, 2 finished), steps recorded, outcomes, whether the finish normalised, T, C, cars_mask, words
 * per line.  _get_state copies the lines of the first `steps` steps ([steps * R][32] float32 words, bits as they are) and the three
 * statistics to device buffers on `stream` (each optional); _set_state puts them back together with the first four info words. */
int crl_car_rollout_get_info(crl_car_rollout *r, int32_t *out8_host);
int crl_car_rollout_get_state(crl_car_rollout *r, int64_t steps, float *lines_out_dev, double *stats_out_dev, void *stream);
int crl_car_rollout_set_state(crl_car_rollout *r, const int32_t *info4_host, int64_t steps, const float *lines_dev, const double *stats_dev, void *stream);

/* ---- car ppo update: the gradient and optimiser step for the car policy's MLP on the device ----------------
 * What "ppo update" is for the LightActorCritic, for the MLP(21, 2) of "car policy" with its Gaussian head.  The MASTER WEIGHTS ARE A
 * CAR POLICY BLOB (CRL_CAR_POLICY_BLOB_FLOATS floats in the layout of "car policy"): handing them to a served policy is
 * crl_car_policy_set_weights(policy, slot, crl_car_ppo_weights_dev(..), 0, stream), a device-to-device copy.  The blob holds 2505
 * parameters (fc1_w, fc1_b, policy_w, value_w, policy_b, value_b, log_std); the two std floats are derived, not trained -- their
 * gradient and Adam moments stay 0 -- and the pad stays 0.  rules.car_ppo_loss_reference (torch float64 autograd) restates the loss,
 * rules.adam_reference the step.
 *
 * Loss.  Per LIVE sample b of the minibatch, with x, u, old_logp, ret as stored and A the advantage as the gather hands it out:
 *   a = fc1(x);  h = max(a, 0) with derivative (a > 0 ? 1 : 0);  mean = policy(h);  v = value(h);
 *   std_d = exp(log_std_d);  zz_d = (u_d - mean_d) / std_d;  logp = sum_d (-0.5 zz_d^2 - log_std_d) - ln(2 pi);  r = exp(logp - old_logp);
 *   policy = -min(r A, clamp(r, 1 - c, 1 + c) A), with g = d policy / d logp = -(A r) if (A >= 0 and r < 1 + c) or (A < 0 and r > 1 - c),
 *     else 0 -- exactly the clipped surrogate of "ppo update", the same branch conditions;
 *   value = 0.5 (ret - v)^2;  entropy = log_std_0 + log_std_1 + (1 + ln(2 pi));
 *   loss = (sum over the LIVE samples of policy + vf * value - ent * entropy) / max(L, 1), L the minibatch's live count.
 * A dead sample contributes nothing to the gradient or to the statistics.  Closed forms:
 *   d loss_b / d mean_d = g zz_d / std_d;   d loss_b / d log_std_d = g (zz_d^2 - 1) - ent;   d loss_b / d v = vf (v - ret).
 * Precision: the hidden layer is float32 (the serving kernel's order: fc1_b[j], then inputs 0..20); from h on, mean, v, logp, r and the
 * three derivative heads are formed in float64 and rounded once to float32; the backward pass through the two layers is float32,
 * da_j = (a_j > 0) ? ((d0 wp0_j + d1 wp1_j) + dv wv_j) : 0.
 * Summation shape, a function of B alone: groups of G = 64 consecutive idx entries, W = min(1024, ceil(B / 64)) workgroups of one
 * wavefront, workgroup w taking groups w, w + W, ... in order.  fc1_w, fc1_b, policy_w and value_w are sums over the samples on
 * v_mfma_f32_16x16x4_f32, the samples as its K dimension: four consecutive samples per instruction (the instruction's own order within
 * the four), the instructions of a group in sample order, a workgroup's groups in order into the same accumulators.  policy_b, value_b
 * and log_std: the UNROUNDED float64 closed forms; lane l adds its samples (entry l of each of the workgroup's groups) in order in
 * float64, then the butterfly of "car policy" over the 64 lanes in float64.  The workgroups' partial sums are added in workgroup
 * order and divided by float32(max(L, 1)) (the five float64 sums: added in float64, divided by L in float64, rounded once).  No
 * floating-point atomics: the same idx gives the same bits on every run.
 * Statistics: the means over the live samples of policy, value, entropy, old_logp - logp and the clipped share (r outside [1 - c,
 * 1 + c]) in float64, the gradient's norm before clipping, the optimiser steps taken, and L.
 * Step: clip by the global norm and Adam by the rule of "ppo update", unchanged, over the 2505 parameters; then
 * std_d = float32(exp(float64(log_std_d))) is rewritten in the master blob on the device (the serving kernel evaluates no exp).
 * Default hyper-parameters of the Python side are common continuous-control practice: clip 0.2, vf 0.5, ent 0.0, lr 3e-4, betas (0.9,
 * 0.999), eps 1e-5, max_grad_norm 0.5. */
typedef struct crl_car_ppo crl_car_ppo;
/* blob_host: a car policy blob; the std floats and the pad are recomputed.  Both moments and the step count start at 0. */
int crl_car_ppo_create(int32_t device, const float *blob_host, crl_car_ppo **out);
void crl_car_ppo_destroy(crl_car_ppo *p);
int crl_car_ppo_set_weights(crl_car_ppo *p, const float *blob_host); /* zeroes the moments and the step count (synchronises) */
int crl_car_ppo_get_weights(crl_car_ppo *p, float *blob_out_host);   /* (synchronises) */
int crl_car_ppo_weights_dev(crl_car_ppo *p, const float **blob_dev);
/* The gradient over the samples idx_dev [count] of a finished storage, at the master weights, on `stream`. */
int crl_car_ppo_grad(crl_car_ppo *p, const crl_car_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper, void *stream);
/* The last gradient, a blob in the weights' layout: its device address and / or a host copy (synchronises). */
int crl_car_ppo_get_grad(crl_car_ppo *p, const float **grad_dev, float *grad_out_host);
int crl_car_ppo_step(crl_car_ppo *p, const crl_ppo_hyper *hyper, void *stream);
/* out8: policy loss, value loss, entropy, approximate KL, clipped share, gradient norm, steps, L (synchronises the device). */
int crl_car_ppo_stats(crl_car_ppo *p, double *out8_host);
/* Resume: the master blob, Adam's moments and the step count, behind / ordered on `stream` (both synchronise with it). */
int crl_car_ppo_get_state(crl_car_ppo *p, float *blob_out_host, float *m_out_host, float *v_out_host, int64_t *steps_out, void *stream);
int crl_car_ppo_set_state(crl_car_ppo *p, const float *blob_host, const float *m_host, const float *v_host, int64_t steps, void *stream);

/* ---- car ppo update, teacher targets: imitation and KL-to-teacher for the car policy's learner ----------------
 * Extends "car ppo update"; nothing in that section changes.  One term is added to d loss / d mean and d loss / d log_std in the heads;
 * everything behind the heads -- the matrix-instruction backward, the five float64 bias sums, the summation shape, the reduce, the
 * optimiser step, the push, resume -- is untouched.  Serves cloning a rule (a second crl_car_driver with RULE_BASED and epsilon 0 writes
 * what it would do into a scratch action array), distilling one network into another (a deterministic crl_car_policy slot writes its mean
 * the same way) and PPO held near a teacher.  rules.car_ppo_teacher_loss_reference (torch autograd) restates the loss.
 *
 * Target of sample b, from row s = idx[b] (the flat t * R + row index; never row b) of two device arrays:
 *   target         float32 [T * R][2]: the teacher's action or mean t_d;
 *   value_targets  float32 [T * R], optional: target_v = value_targets[s] in place of the stored return (a teacher's critic).
 * A sample is TAUGHT iff it is live and both floats of its target are finite.  An untaught sample has teacher term 0, teacher
 * derivatives 0 and teacher statistics 0, by selection, not by a product with 0: a NaN target never reaches a sum.
 * Teacher spread: two host floats teacher_log_std[2] = lsq_d give sq_d = exp(2 (double) lsq_d), formed in float64 from the float32
 * values; point = 1 sets sq_d = 0 (and lsq_d is not read): a deterministic teacher such as RULE_BASED.
 * Kinds.  With mean_d, std_d, log_std_d the learner's as "car ppo update" forms them in float64, dm_d = mean_d - t_d and
 * var_d = std_d std_d:
 *   CRL_CAR_TEACHER_CE    term = ((log_std_0 + (sq_0 + dm_0^2) / (2 var_0)) + (log_std_1 + (sq_1 + dm_1^2) / (2 var_1))) + ln(2 pi)
 *                         = E_q[-log p] for the teacher q = N(t, sq) -- for a point teacher the Gaussian negative log-likelihood of t;
 *                         t_mean_d = dm_d / var_d;   t_ls_d = 1 - (sq_d + dm_d^2) / var_d;
 *   CRL_CAR_TEACHER_MSE   term = 0.5 (dm_0^2 + dm_1^2);   t_mean_d = dm_d;   t_ls_d = 0.
 * Loss, per LIVE sample:   loss_b = policy_term * policy + vf * value - ent * entropy + coef * [taught] * term,   the sum divided by
 * max(L, 1) as before;
 *   policy_term in {0, 1}: at 0 the rule sets g = d policy / d logp = 0 -- pure imitation; the stored advantage and old log-prob then
 *   play no part in the gradient (they still enter the existing statistics);  coef >= 0, finite;
 *   value = 0.5 (target_v - v)^2.
 * Closed forms, float64, rounded once to float32, the teacher term added last:
 *   d loss_b / d mean_d = (the expression of "car ppo update") + coef t_mean_d;
 *   d loss_b / d log_std_d = (the expression) + coef t_ls_d;     d loss_b / d v = vf (v - target_v).
 * With coef = 0, policy_term = 1 and no value targets the gradient therefore equals crl_car_ppo_grad's as numbers.
 * Statistics: the six of "car ppo update" as always, and four more, float64 sums in the summation shape of the six (per lane over
 * its samples, the butterfly, the workgroups in order): term; kl = term - ((lsq_0 + lsq_1) + (1 + ln(2 pi))) for CE with point = 0
 * (= KL(q || p)), 0 otherwise; abs_err = (|dm_0| + |dm_1|) / 2 -- the three as means over the Lt taught samples, divisor
 * max(Lt, 1) --; and taught = Lt / max(L, 1).
 * The kernels: the teacher instantiations of the gradient and statistics kernels; the plain instantiations are what crl_car_ppo_grad
 * launches, with no teacher load, select or statistic in them.  A lane loads its sample's 8-byte target row and, when value targets
 * are given, their 4 bytes.  The same launches, no floating-point atomics, the same call gives the same bits on every run, nothing
 * synchronises, all work is ordered on the caller's stream. */
enum crl_car_teacher_kind { CRL_CAR_TEACHER_CE = 0, CRL_CAR_TEACHER_MSE = 1 };
typedef struct crl_car_ppo_teacher {
    const float *target_dev;          /* [rows][2] */
    const float *value_targets_dev;   /* [rows] or null = the stored returns */
    int64_t rows;                     /* must equal T * R of the rollout */
    float teacher_log_std[2];         /* read when point = 0 */
    int32_t point;                    /* 1: a deterministic teacher, sq_d = 0 */
    int32_t kind;                     /* enum crl_car_teacher_kind */
    float coef;
    int32_t policy_term;
} crl_car_ppo_teacher;
/* crl_car_ppo_grad with a teacher; crl_car_ppo_step, _stats, _get_grad and _weights_dev work behind it as behind crl_car_ppo_grad.  The
 * teacher's arrays are the caller's and must stay valid until the launches have run.  Refuses (CRL_EINVAL, before any GPU call, the
 * learner as it was): everything crl_car_ppo_grad refuses; a null teacher or target; rows != T * R; a kind outside the enum; point or
 * policy_term outside {0, 1}; a coef that is not finite and >= 0; a teacher_log_std that is not finite when point = 0; a target that
 * is not 8-byte aligned or value targets that are not 4-byte aligned. */
int crl_car_ppo_grad_teacher(crl_car_ppo *p, const crl_car_rollout *rollout, const int64_t *idx_dev, int64_t count, const crl_ppo_hyper *hyper,
                             const crl_car_ppo_teacher *teacher, void *stream);
/* out4_host: term, kl, abs_err, taught of the last crl_car_ppo_grad_teacher.  Synchronises the device, like crl_car_ppo_stats.  Refuses
 * (CRL_EINVAL) when the learner's last gradient was a plain crl_car_ppo_grad's, or when it has none. */
int crl_car_ppo_teacher_stats(crl_car_ppo *p, double *out4_host);

/* ---- car league: per-env opponents for car 1 and race books on the device --------------
 * What "league" and "league ledger" are for cPongTournament, for a two-car CarRacing context: a pool of opponents, a per-env draw of
 * who drives car 1, and books of how car 0 (the caller's car, the seat make_competitive_car_racing gives its agent,
 * car_racing/make_competitive_car_racing.py:10-58) fares against each of them.  An object beside the context, a crl_car_policy and a
 * crl_car_driver of that context: it reads the step's rewards and done flags and WRITES column 1 of both objects' device assignment
 * arrays, nothing else of them; column 0 is never touched.  All work is ordered on the caller's stream; no call synchronises with the
 * host, the getters hand over device memory (crl_car_league_get_pool returns host values and makes no GPU call).
 * rules.car_league_reference and rules.car_league_draw_reference restate this section in numpy.
 *
 * Pool.  Up to CRL_LEAGUE_MAX_AGENTS entries (kind, slot), append-only: kind CRL_CAR_LEAGUE_NETWORK names a network slot of the
 * policy, kind CRL_CAR_LEAGUE_STYLE a style slot of the driver.  Serving agent a means: policy assignment[e][1] = slot and driver
 * assignment[e][1] = -1 for a network, the other way round for a style.
 *
 * State.  Per env: agent int32 (the pool entry that drives car 1; -1 until the first draw), ret float32 [2] (the running episode's
 * summed step rewards of car 0 and car 1), len int32 (its steps), draw_ctr uint32.  Per agent: CRL_CAR_LEAGUE_COUNTERS int64 counters,
 * laid out [counter][CRL_LEAGUE_MAX_AGENTS] in the order of enum crl_car_league_counter.  A weight table uint32
 * w[CRL_LEAGUE_MAX_AGENTS]: 1 for an entry when it enters the pool, 0 beyond the pool.
 *
 * crl_car_league_step, one launch with one lane per env, enqueued behind the crl_step that wrote rewards and done:
 *   1. ret[c] = ret[c] + reward[e][c] for c = 0, 1 in float32, one rounding per add, in step order; len += 1;
 *   2. where done[e] != 0 the episode is credited to agent[e], the entry that DROVE it: episodes += 1; one of wins (ret[0] > ret[1]) /
 *      losses (ret[0] < ret[1]) / draws (otherwise: equal, or a NaN on either side) += 1; return_sum += q(ret[0]);
 *      opponent_return_sum += q(ret[1]); length_sum += len; then ret = len = 0.  q(x) = llrint(clamp((double)x * 256.0, -2^62, 2^62))
 *      (round to nearest, ties to even) for a finite x and 0 otherwise: returns in units of 1/256.  An agent outside [0, agents) (-1:
 *      no draw yet) is credited nowhere.  All sums are 64-bit integer atomics, reduced per wavefront by the keys present: the totals do
 *      not depend on the order in which wavefronts arrive;
 *   3. where done[e] != 0 and redraw != 0: a weighted draw by the rule of "ledger draws" with CRL_CAR_LEAGUE_DOMAIN in place of
 *      CRL_LEDGER_DOMAIN_OPPONENT (key = the league's seed, gid = the context's env_id_base + e, n = draw_ctr[e]); then agent[e] = the
 *      drawn entry, draw_ctr[e] += 1, and column 1 of row e of both assignment arrays is written as above.  A table that sums to 0
 *      (or past 2^32 - 1) keeps the env's agent, counter and assignments.  The next crl_car_policy_act / crl_car_driver_act on the
 *      stream serves the new opponent from the first step of the new episode (crl_step has reset the env already).
 * A draw depends on (seed, global env id, counter, table) alone: shards that hold the same table draw what the whole batch would.
 * PFSP weights: the rule of "PFSP weights" over the planes episodes, wins and draws. */
#define CRL_CAR_LEAGUE_DOMAIN 0x43524C47u /* "CRLG" */
#define CRL_CAR_LEAGUE_COUNTERS 7
enum crl_car_league_counter { CRL_CAR_LEAGUE_EPISODES = 0, CRL_CAR_LEAGUE_WINS = 1, CRL_CAR_LEAGUE_LOSSES = 2, CRL_CAR_LEAGUE_DRAWS = 3,
                              CRL_CAR_LEAGUE_RETURN_SUM = 4, CRL_CAR_LEAGUE_OPPONENT_RETURN_SUM = 5, CRL_CAR_LEAGUE_LENGTH_SUM = 6 };
enum crl_car_league_kind { CRL_CAR_LEAGUE_NETWORK = 0, CRL_CAR_LEAGUE_STYLE = 1 };
typedef struct crl_car_league crl_car_league;
/* A league for the envs of the two-car CarRacing context `ctx` and a policy and a driver of THAT context; all three must outlive it.
 * The pool is empty.  Refuses (CRL_EINVAL, before any GPU call) a null argument, a Pong context, a one-car context and a policy or
 * driver of another context. */
int crl_car_league_create(crl_ctx *ctx, crl_car_policy *policy, crl_car_driver *driver, uint64_t seed, crl_car_league **out);
void crl_car_league_destroy(crl_car_league *l);
/* Appends (kind, slot) to the pool; its id goes to *id_out (optional) and its weight becomes 1 in stream order.  Refuses a kind
 * outside the enum, a slot outside [0, CRL_CAR_POLICY_SLOTS) / [0, CRL_CAR_DRIVER_SLOTS) and a 17th entry. */
int crl_car_league_add_agent(crl_car_league *l, int32_t kind, int32_t slot, int32_t *id_out, void *stream);
/* The pool (host values, no GPU call): its size, and kinds / slots as int32 [CRL_LEAGUE_MAX_AGENTS] (-1 beyond the pool); each optional. */
int crl_car_league_get_pool(crl_car_league *l, int32_t *agents_out, int32_t *kinds_out, int32_t *slots_out);
/* A fresh draw (step 3) for EVERY env, e.g. after crl_reset. */
int crl_car_league_draw_all(crl_car_league *l, void *stream);
/* New key for the draws, every draw_ctr back to 0 (results, weights and assignments stay). */
int crl_car_league_seed(crl_car_league *l, uint64_t seed, void *stream);
/* Zeroes the counters and every env's ret / len (weights, key, draw counters and assignments stay). */
int crl_car_league_reset(crl_car_league *l, void *stream);
/* Zeroes the counter column of pool entry `agent` (a slot that took a newer snapshot starts its record over). */
int crl_car_league_reset_agent(crl_car_league *l, int32_t agent, void *stream);
/* w_host: uint32 [count] on the HOST, count == the pool's size, summing to a value in [1, 2^32) (read before the call returns). */
int crl_car_league_set_weights(crl_car_league *l, const uint32_t *w_host, int32_t count, void *stream);
/* w_out_dev: uint32 [CRL_LEAGUE_MAX_AGENTS] on the device. */
int crl_car_league_get_weights(crl_car_league *l, uint32_t *w_out_dev, void *stream);
/* The PFSP table from counters_dev (int64 [CRL_CAR_LEAGUE_COUNTERS][CRL_LEAGUE_MAX_AGENTS] on the device, e.g. all-reduced over the
 * shards) or from the league's own counters when NULL; mode, exponent and floor as crl_ledger_pfsp_weights takes and refuses them. */
int crl_car_league_pfsp_weights(crl_car_league *l, const int64_t *counters_dev, int32_t mode, int32_t exponent, uint32_t floor, void *stream);
/* Counters as int64 [CRL_CAR_LEAGUE_COUNTERS][CRL_LEAGUE_MAX_AGENTS], device memory. */
int crl_car_league_get_counters(crl_car_league *l, int64_t *counters_out_dev, void *stream);
int crl_car_league_set_counters(crl_car_league *l, const int64_t *counters_dev, void *stream);
/* Checkpoints / tests: the per-env values on the device, each optional: agent int32 [N], ret float32 [N][2], len int32 [N], draw_ctr
 * uint32 [N].  _set_env_state with an agent array also writes column 1 of both assignment arrays for every env whose agent lies in the
 * pool, so that the opponent served is the one the books will credit. */
int crl_car_league_get_env_state(crl_car_league *l, int32_t *agent_out_dev, float *ret_out_dev, int32_t *len_out_dev, uint32_t *draw_ctr_out_dev,
                                 void *stream);
int crl_car_league_set_env_state(crl_car_league *l, const int32_t *agent_dev, const float *ret_dev, const int32_t *len_dev,
                                 const uint32_t *draw_ctr_dev, void *stream);
/* The agent array: int32 [N] on the device. */
int crl_car_league_get_assignment(crl_car_league *l, int32_t *agent_out_dev, void *stream);
/* The per-step call described above: rewards_dev float32 [N][2] and done_dev uint8 [N] as crl_step wrote them. */
int crl_car_league_step(crl_car_league *l, const float *rewards_dev, const uint8_t *done_dev, int32_t redraw, void *stream);

/* Text of the most recent failing call: of the calling thread (any call, crl_create included), or of one context. */
const char *crl_last_error(void);
const char *crl_ctx_last_error(const crl_ctx *ctx);
const char *crl_version(void);

/* Device self-test of include/crl_rot.h (no context needed): evaluates crl_sincosf on the float32 bit patterns
 * [first_bits, first_bits + count) that lie in its domain and compares each result with the double-double evaluation of
 * include/crl_f64.h rounded once to float32.  out5_host: [0] arguments tested, [1] sine results that are not the correctly
 * rounded float32, [2] cosine likewise, [3] results too close to a rounding boundary for the double-double bound to decide,
 * [4] first mismatching bit pattern + 1 (0 = none).  The whole space (first_bits 0, count 2^32) takes a few seconds.
 * Replaces nothing in the reference: Box2D calls the host libm's sinf / cosf (b2Math.h b2Rot::Set, via box2d-py,
 * car_racing/car_racing_multi_players.py:600); this pins the one evaluation both sides of the parity tests share. */
int crl_selftest_sincosf(int32_t device, uint64_t first_bits, uint64_t count, uint64_t *out5_host);

#ifdef __cplusplus
}
#endif
#endif /* CRL_H_ */
