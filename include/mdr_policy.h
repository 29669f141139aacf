/*
 * mdr_policy.h - fused policy forward + action sampling for rollout collection.
 *
 * Replaces, for all agents of all envs at once, what the reference does per agent and step on the CPU:
 *   PPO.select_action (agents/ppo.py:68-75): actor_net(state) -> Categorical(action_prob).sample() -> (action, prob)
 *   Actor.forward      (agents/network.py:14-33): Linear/ReLU stack (two hidden layers) with a softmax head, 2 actions
 *
 * One kernel: observation rows [A][F] -> layer 1 -> ReLU -> layer 2 -> ReLU -> logits -> softmax -> sample.
 * The two dense layers run on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma chain, no
 * reduced precision), the hidden activations never leave the registers, biases ride along as one extra input / hidden
 * unit that is constant 1.  The weights are handed over pre-arranged in MFMA fragment order (mdr_actor_pack_* below
 * describe it; mdr_amd/policy.py builds it from a torch state_dict).
 *
 * Part of libmdr_hip.so; plain C ABI, device pointers, stream-ordered, never synchronises.
 */
#ifndef MDR_POLICY_H
#define MDR_POLICY_H

#include <stdint.h>

#include "mdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_ACTOR_MAX_HIDDEN 127 /* per hidden layer: 127 units + the constant-1 unit fill four 32-row MFMA blocks */

enum mdr_actor_layout {
  MDR_ACTOR_FRAG32 = 0, /* v_mfma_f32_32x32x2_f32: 32 agents per wavefront, any num_state that fits the LDS */
  MDR_ACTOR_FRAG16 = 1, /* v_mfma_f32_16x16x4_f32: 16 agents per wavefront, hidden units padded to 112 instead of 128 rows and a
                           quarter of the accumulator registers; num_state <= 128 (16 feature registers per lane up to 64
                           features, 32 beyond - observations with the optional message columns, utils.py:858-866) */
  MDR_ACTOR_BF16X3 = 2, /* v_mfma_f32_16x16x32_bf16 on operands split into bf16 head + tail (x = xh + xl): w x ~ wh xh + wl xh +
                           wh xl, fp32 accumulation - 16 significand bits per operand instead of 24 (probabilities within ~1e-5
                           of the fp32 forward) at 16 / 3 times the fp32 matrix rate; num_state <= 128 (mdr_actor_sample; 64 through
                           mdr_env_actor_sample).  frag1 / frag2 hold bf16 */
  MDR_ACTOR_FRAG16T = 3 /* MDR_ACTOR_FRAG16 for hidden layers of 97..100 units (the reference's [100, 100]): six 16-row blocks on
                           v_mfma_f32_16x16x4_f32 and the last 1..4 units of either layer on v_mfma_f32_4x4x1_16B_f32 (exact fp32,
                           a third of the time of the block it replaces): ~9 % fewer matrix cycles per agent */
};

typedef struct mdr_actor {
  uint32_t struct_size;
  int32_t layout;      /* mdr_actor_layout: how frag1 / frag2 / wdiff are arranged */
  int32_t num_state;   /* F: floats per observation row */
  int32_t hidden1;     /* units of hidden layer 1 (<= MDR_ACTOR_MAX_HIDDEN) */
  int32_t hidden2;     /* units of hidden layer 2 (<= MDR_ACTOR_MAX_HIDDEN) */
  int32_t greedy;      /* 0: action ~ Categorical(softmax) (PPOAgent.act, agents/rl_controllers.py:28-36); 1: action = argmax of the two
                          outputs (DQNAgent.act, rl_controllers.py:53-60: the same Linear/ReLU stack read as Q-values), no draw */
  int32_t feature_order; /* which input feature column k of W1 multiplies: 0 = MDR_FEATURES_NORMSTATE, normStateDict's own order
                            (mdr_actor_sample); 1 = MDR_FEATURES_OBSERVE, the order mdr_env_actor_sample stages the observation
                            in - the messages first (k = 4 m + field), then the own features in normStateDict order (k = M + i,
                            M = observe_msg_floats): W1's columns permuted with k -> normStateDict index (k < M ? own + k : k - M),
                            own = num_state - M */
  int32_t observe_msg_floats; /* MDR_FEATURES_OBSERVE: M = 4 * nb_comm message floats lead the staged row (40 for the reference's
                                 default 10 neighbours; 0 = no messages) */
  /* device, MFMA fragment order.  W1z / W2z / W3z: the weight matrices zero-padded to 128 rows / columns.
   * MDR_ACTOR_FRAG32 (S1 = ceil((F + 1) / 2), S2 = mdr_actor_steps2, r = lane & 31, h = lane >> 5) carries the biases as a
   * constant-1 input feature / hidden unit:  W1e = [[W1 b1] [0 1]],  W2e = [[W2 b2] [0 1]],  W3e = [W3 b3]:
   *   frag1[s][lane][mb < 4]  = W1e[32 mb + r][h S1 + s]
   *   frag2[q][lane][mb < 4]  = W2e[32 mb + r][k2],  k2 = 32 (q >> 4) + (q & 3) + 8 ((q >> 2) & 3) + 4 h  (the accumulator row the lane holds)
   *   wdiff[mb < 4][reg < 16][h] = W3e[0][row] - W3e[1][row],  row = 32 mb + (reg & 3) + 8 (reg >> 2) + 4 h      (128 floats)
   * MDR_ACTOR_FRAG16 (S1 = ceil(F / 4), S2 = 4 floor(H1 / 16) + ceil((H1 % 16) / 4), r = lane & 15, g = lane >> 4); the biases start
   * the accumulators.  Hidden-1 units of a partial last 16-row block are stored transposed - unit 16 b + j in row (of W1z, b1) /
   * column (of W2z) 16 b + 4 (j % 4) + j / 4 - so that the block's first ceil((H1 % 16) / 4) k-steps of layer 2 carry them all:
   *   frag1[s][lane][mb < 8]  = W1z[16 mb + r][g S1 + s]
   *   frag2[q][lane][mb < 8]  = W2z[16 mb + r][16 (q >> 2) + 4 g + (q & 3)]
   *   wdiff (388 floats) = d[mb < 8][reg < 4][g < 4] | b1[mb][g][reg] | b2[mb][g][reg] | b3[0] - b3[1] | 0 0 0,
   *                        d = W3z[0][row] - W3z[1][row],  b1 / b2 at row (0 past H),  row = 16 mb + 4 g + reg
   * MDR_ACTOR_FRAG16T: as MDR_ACTOR_FRAG16 with S2 = 25, except slot mb = 6 of every fragment and the tail's biases / head weights,
   * u = 96 + (lane & 3) (zero past the layer's units):
   *   frag1[s][lane][6] = W1[u][g S1 + s]      frag2[q < 24][lane][6] = W2[u][16 (q >> 2) + 4 g + (q & 3)]
   *   frag2[24][lane][mb < 6] = W2z[16 mb + r][96 + g]      frag2[24][lane][6] = W2[u][96 + g]
   *   d[6][reg][g] = (g == 0) (W3[0][96 + reg] - W3[1][96 + reg]),  b1 / b2 [6][g][reg] = (g == 0) b[96 + reg]
   * MDR_ACTOR_BF16X3 (S1 = ceil(F / 32), S2 = 4, r = lane & 15, g = lane >> 4, fragments of 8 bf16, t = 0 head / 1 tail):
   *   frag1[s][mb < 8][t][lane][j < 8] = split_t(W1z[16 mb + r][(4 s + g) 8 + j])
   *   frag2[s][mb < 8][t][lane][j < 8] = split_t(W2z[16 mb + r][16 (2 s + (j >> 2)) + 4 g + (j & 3)])
   *   wdiff as MDR_ACTOR_FRAG16;  split_0(w) = bf16(w), split_1(w) = bf16(w - split_0(w)), round to nearest even */
  const void *frag1;
  const void *frag2;
  const float *wdiff;  /* 128 floats (FRAG32) or 388 */
} mdr_actor_t;

int64_t mdr_actor_steps1(int32_t layout, int32_t num_state);        /* S1 */
/* S1 of an actor packed with feature_order = 1 (MDR_FEATURES_OBSERVE) for the exact-fp32 layouts: the k-steps its observe -> act
 * kernel is compiled for - 13 (num_state <= 52, the default 51 included), 15 (<= 60) or 16 (<= 64); W1 columns past num_state are
 * zeros.  Every other (layout, order): mdr_actor_steps1.  frag1 then holds S1 * (mdr_actor_frag1_floats / mdr_actor_steps1) units. */
int64_t mdr_actor_steps1_order(int32_t layout, int32_t num_state, int32_t feature_order);
int64_t mdr_actor_steps2(int32_t layout, int32_t hidden1);          /* S2 */
int64_t mdr_actor_frag1_floats(int32_t layout, int32_t num_state);  /* size of frag1 in 4-byte units */
int64_t mdr_actor_frag2_floats(int32_t layout, int32_t hidden1);    /* size of frag2 in 4-byte units */

/* For every agent a < nb_agents: probs = softmax(actor(obs[a])), u = Philox4x32-10(key = seed, counter = (a, step, stream))
 * uniform in (0,1), action = u < probs[0] ? 0 : 1  (Categorical(probs).sample()), a_prob = probs[action].  The counter is (a low word,
 * a high word, step low word + *step_dev, TAG_ACTION ^ step high word), u = min(((float)(x >> 8) + 0.5f) * 2^-24, 0x1.fffffep-1f) of
 * the first output word x: the clamp keeps the top cell (x >> 8 == 0xFFFFFF, whose centre rounds to 1.0f) below 1, so an action of
 * probability 0 is never drawn.  `step_dev` is added to the low word of `step` modulo 2^32 and does not carry into the high word.
 * `obs`: observation rows [nb_agents][F] when obs_plane_stride == 0 (mdr_env_obs_vector MDR_OBS_ROWS), or feature planes
 * [F][obs_plane_stride] with obs_plane_stride >= nb_agents (MDR_OBS_PLANES: the lanes of a wavefront then read consecutive
 * floats instead of one cache line each).  `action` uint8 [nb_agents], `a_prob` float [nb_agents] (may be NULL), `probs`
 * float [nb_agents][2] (may be NULL).  `step_dev` (device int32, may be NULL) is added to `step` on the device - point it at
 * the time index of mdr_buffers_t.cursor ([1]) so that a captured launch draws fresh numbers at every replay.  Returns 0, or -1 (invalid argument) / -3 (HIP error) / -4 (shape without a kernel). */
int mdr_actor_sample(const mdr_actor_t *actor, const float *obs, int64_t obs_plane_stride, int64_t nb_agents, uint64_t seed,
                     uint64_t step, const int32_t *step_dev, uint8_t *action, float *a_prob, float *probs, void *stream);

/* Observe -> act in ONE kernel (SURVEY 8f-1 + 8f-2 fused): what train_ppo.py:69-75 does per agent - utils.normStateDict(obs_dict[i]) then
 * PPO.select_action - for every agent of every env, WITHOUT materialising the 204-byte observation rows: each wavefront stages the
 * compact state of its 32 (16) consecutive houses and their 5 + 5 circular neighbours in LDS (own features and SingleHouse.message
 * records, the very arithmetic of mdr_env_obs_vector), and the matrix-core forward reads its B operand from there.  Draws, outputs and
 * `step_dev` as mdr_actor_sample (agent index = env * nb_houses + house).  Covers the reference's DEFAULT observation only - every
 * optional state / message column off, agents_comm_mode "neighbours" with nb_agents_comm = 10, no link defects (spec says which; 51
 * features, hence nb_houses >= 11) - with unsharded houses and an actor packed as MDR_ACTOR_FRAG16 or MDR_ACTOR_BF16X3 in
 * MDR_FEATURES_OBSERVE order; anything else returns MDR_ERR_UNSUPPORTED (-4): fall back to mdr_env_obs_vector + mdr_actor_sample.
 * Any cluster size: tiles of 32 (16) consecutive agents may start anywhere in an env and span several (the reference trains with 20
 * houses and deploys with 50); nb_houses % 32 == 0 takes a leaner staging path.
 * `rows_out` (may be NULL; 16-byte aligned for the wide-store path, else 4-byte stores): the observation rows themselves, float [nb_agents][51] in normStateDict order - bit for
 * bit what mdr_env_obs_vector(MDR_OBS_ROWS) writes - copied out of the staged window on the side, for callers that keep the `state` of
 * every transition (train_ppo.py:87-98): the rows are then written once and never read back by the policy. */
int mdr_env_actor_sample(mdr_env_t *env, const mdr_obs_spec_t *spec, const mdr_actor_t *actor, uint64_t seed, uint64_t step,
                         const int32_t *step_dev, uint8_t *action, float *a_prob, float *probs, float *rows_out, void *stream);

/* The same for senders that are NOT the circular neighbours: a static link table (spec->links: agents_comm_mode closed_groups /
 * random_fixed / neighbours_2D, ClusterHouses.build_agent_comm_links env 806-902) or random_sample (spec->random_links, env 976-983:
 * nb_comm distinct senders drawn per house and step).  The call first writes every house's SingleHouse.message record into
 * `msg_scratch` (device float [nb_envs][nb_houses][4], 16-byte aligned; mdr_env_obs_messages' kernel) and - random_sample - this step's
 * senders into `senders_scratch` (device int32 [nb_envs][nb_houses][nb_comm], the draws of mdr_env_comm_draws; may be NULL otherwise);
 * the actor kernel then stages one lane per agent and GATHERS its nb_comm records through the table.  Same draws, outputs and
 * `rows_out` as mdr_env_actor_sample (rows bit for bit those of mdr_env_obs_vector); the optional MESSAGE columns stay unsupported
 * (-4: with 10 senders they do not fit the 64 features of a staged row).  Circular neighbours are accepted too (NULL links). */
int mdr_env_actor_sample_links(mdr_env_t *env, const mdr_obs_spec_t *spec, const mdr_actor_t *actor, float *msg_scratch,
                               int32_t *senders_scratch, uint64_t seed, uint64_t step, const int32_t *step_dev, uint8_t *action,
                               float *a_prob, float *probs, float *rows_out, void *stream);

/* The Monte-Carlo return scan of PPO.update (agents/ppo.py:123-134) for every agent at once: backwards over t,
 * R <- reward[t] + gamma * (done[t] ? bootstrap[t] : R).  `reward`, `out` float [nb_steps][nb_agents]; `done` uint8 of that
 * shape or NULL (no restarts); `bootstrap` float of that shape (the critic's value of the next state where done) or NULL
 * (restart from 0: zero_eoepisode_return). */
int mdr_discounted_returns(const float *reward, const uint8_t *done, const float *bootstrap, float gamma, int32_t nb_steps,
                           int64_t nb_agents, float *out, void *stream);

/* ---- TarMAC-PPO actor (agents/network.py:103-238, TarMAC_Comm / TarMAC_Actor): the attention and the head's last step.  The
 * actor's five small per-agent MLPs are either library GEMMs on the caller's side (mdr_amd/tarmac.py TarMACActor; these two kernels
 * are what no GEMM covers) or the matrix-core kernels of mdr_tarmac_actor_sample below, which runs the whole actor. */
enum mdr_tarmac_precision {
  MDR_TARMAC_FP32 = 0,  /* exact fp32 MLPs: the frag_* arrays hold floats in the order given at mdr_tarmac_actor_t */
  MDR_TARMAC_BF16X3 = 1 /* every product of the MLPs' matrix layers as wh xh + wl xh + wh xl on operands split into a bf16 head and
                           tail, fp32 accumulation from the fp32 bias (as MDR_ACTOR_BF16X3: probabilities within the bf16x3 contract,
                           2e-3 relative + 2e-5, of the fp64 forward); activations, the head's last layer, the softmax, the draw and
                           the attention stay fp32.  The frag_* arrays hold bf16 fragments */
};

enum mdr_tarmac_mode {
  MDR_TARMAC_NEIGHBOURS = 0, /* tarmac_comm_mode "neighbours": the circular band of make_masks (network.py:146-165) */
  MDR_TARMAC_NONE = 1        /* "none": an all-zero mask WITHOUT diagonal - the reference's 0 / 0 -> NaN -> 0: out = 0 */
};

/* Banded masked attention of TarMAC_Comm.forward (network.py:187-198) for every agent a = env * nb_houses + house at once.
 * `query` / `key` float rows of num_key floats, `value` / `out` rows of num_value floats, each with its own leading dimension in
 * floats (ldq, ldk, ldv, ldo): one packed projection buffer [A][K + K + V] can be handed over without copies, and `out` may be
 * a column block of a wider buffer (the other columns are not touched).  c = min(nb_comm, nb_houses - 1); receiver r hears itself
 * and the senders r + o (mod nb_houses) for the first c offsets of +1, -1, +2, -2, ... :
 *   score_s = query_r . key_s / sqrt(num_key),  attn = softmax over those c + 1 senders,  out_r = sum_s attn_s value_s.
 * The maximum subtracted inside the softmax is the band's own (the reference subtracts the maximum of the unmasked row: the same
 * quotient except where the reference underflows to 0 / 0 -> 0).  c = 0: out = value, bit for bit.
 * defect_prob > 0 (make_masks 159-165): sender s is silenced for every receiver but itself iff u < defect_prob in float32, u the
 * uniform of mdr_actor_sample taken of word `hop` (0..3) of Philox4x32-10 with key = seed and counter = (s low word, s high word,
 * step low word + *step_dev, 0x544D4331 ^ step high word), s the sender's agent index in the whole batch: one draw per env, step and
 * hop.  defect_prob == 0 draws nothing.
 * Limits: num_key a multiple of 4 and <= 32, num_value a multiple of 4 and <= 64, c <= 64 after the clamp (-4 otherwise); all four
 * pointers 16-byte aligned and all leading dimensions multiples of 4 floats (-1 otherwise).  Every element of every out row is
 * written, in mode MDR_TARMAC_NONE too.  Returns 0, or -1 / -3 / -4 with nothing launched. */
int mdr_tarmac_comm(const float *query, int64_t ldq, const float *key, int64_t ldk, const float *value, int64_t ldv, int32_t nb_envs,
                    int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, float defect_prob,
                    uint64_t seed, uint64_t step, const int32_t *step_dev, int32_t hop, float *out, int64_t ldo, void *stream);

/* The gradient of the attention above (the training path).  The operands up to `hop` are the forward call's; `out` is what that call wrote,
 * `grad_out` (rows of num_value floats) the gradient g of a scalar loss with respect to it.  With S(r) the live senders of receiver r
 * and p_rs its softmax weights:
 *   delta_r = g_r . out_r,   ds_rs = p_rs (g_r . value_s - delta_r),
 *   grad_query_r = sum_{s in S(r)} ds_rs key_s / sqrt(num_key),   grad_key_s = sum_{r: s in S(r)} ds_rs query_r / sqrt(num_key),
 *   grad_value_s = sum_{r: s in S(r)} p_rs g_r
 * (sender s is heard by the receivers s - o).  The dead-sender flags are redrawn from the same Philox counter: a call with the forward's
 * (seed, step, *step_dev, hop) sees the forward's mask, no mask is stored.  Every element of the three results is written (the caller
 * does not zero them), each through its own leading dimension; the sums are gathered per row in a fixed order, without floating-point
 * atomics, so the same operands give the same bits.  MDR_TARMAC_NONE writes exact zeros; c = 0: grad_value = grad_out bit for bit
 * and grad_query = grad_key = 0.  `workspace`: 16-byte aligned device memory of mdr_tarmac_comm_backward_workspace_bytes() bytes,
 * owned by the caller, contents irrelevant before and after (not needed, and may be NULL, in mode MDR_TARMAC_NONE).  Limits and
 * status codes as the forward's, for all eight pointers and leading dimensions; a missing or unaligned workspace is -1.  Returns 0,
 * or -1 / -3 / -4 with nothing launched and nothing written. */
int mdr_tarmac_comm_backward(const float *query, int64_t ldq, const float *key, int64_t ldk, const float *value, int64_t ldv,
                             int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode,
                             float defect_prob, uint64_t seed, uint64_t step, const int32_t *step_dev, int32_t hop, const float *out,
                             int64_t ldo, const float *grad_out, int64_t ldg, float *grad_query, int64_t ldgq, float *grad_key,
                             int64_t ldgk, float *grad_value, int64_t ldgv, void *workspace, void *stream);

/* Bytes of `workspace` for nb_agents = nb_envs * nb_houses agents (one float4 of softmax statistics per receiver); -1 for
 * negative or zero sizes of the rows. */
int64_t mdr_tarmac_comm_backward_workspace_bytes(int64_t nb_agents, int32_t num_key, int32_t num_value);

/* The two calls above with the Philox key of the dead-sender draw read from device memory when the kernel runs: `key_dev` int32 [2] =
 * (seed low word, seed high word), the convention of mdr_minibatch_permutation_keyed, in place of `seed`; every other argument, the
 * counter (sender lo, sender hi, step low word + *step_dev, 0x544D4331 ^ step high word, word `hop`), the limits and the status codes
 * are the by-value calls'.  A call whose `key_dev` holds the two words of `seed` gives the by-value call's bits, so a captured node
 * need not bake the seed in (graph_update.py: TarMACPPOUpdateGraph).  defect_prob == 0 never reads `key_dev`; a NULL `key_dev` is -1
 * with nothing launched and nothing written. */
int mdr_tarmac_comm_keyed(const float *query, int64_t ldq, const float *key, int64_t ldk, const float *value, int64_t ldv,
                          int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode,
                          float defect_prob, const int32_t *key_dev, uint64_t step, const int32_t *step_dev, int32_t hop, float *out,
                          int64_t ldo, void *stream);
int mdr_tarmac_comm_backward_keyed(const float *query, int64_t ldq, const float *key, int64_t ldk, const float *value, int64_t ldv,
                                   int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm,
                                   int32_t mode, float defect_prob, const int32_t *key_dev, uint64_t step, const int32_t *step_dev,
                                   int32_t hop, const float *out, int64_t ldo, const float *grad_out, int64_t ldg, float *grad_query,
                                   int64_t ldgq, float *grad_key, int64_t ldgk, float *grad_value, int64_t ldgv, void *workspace,
                                   void *stream);

/* ---- The two non-banded masks of make_masks (network.py:138-177), tarmac_comm_mode "all" and "random_sample": entry points of
 * their own (csrc/mdr_tarmac_gather.hip); enum mdr_tarmac_mode and the calls above keep their two banded modes. */
enum mdr_tarmac_gather_mode {
  MDR_TARMAC_ALL = 0,          /* "all": receiver r attends to all nb_houses agents of its env, itself included; nothing is drawn,
                                  nb_comm is ignored */
  MDR_TARMAC_RANDOM_SAMPLE = 1 /* "random_sample": r attends to itself and to c = min(nb_comm, nb_houses - 1) distinct other agents of
                                  its env, uniform among the c-subsets of the others */
};

/* mdr_tarmac_comm for these masks: the same operands (rows, leading dimensions, packed buffers and column blocks in place), limits
 * (num_key a multiple of 4 <= 32, num_value a multiple of 4 <= 64, 16-byte alignment), status codes, `step_dev` and `hop`, without
 * defect_prob - the reference applies comm_defect_prob in mode "neighbours" only (network.py:159-163), these modes have no defects.
 * score_s = query_r . key_s / sqrt(num_key), softmax over the receiver's senders with the maximum over THOSE senders subtracted (as
 * mdr_tarmac_comm), out_r = sum_s attn_s value_s; MDR_TARMAC_ALL sums the senders in ascending house order, MDR_TARMAC_RANDOM_SAMPLE
 * the receiver first, then the drawn senders in the order drawn.  nb_houses == 1 or c == 0: out = value, bit for bit.
 * The draw of MDR_TARMAC_RANDOM_SAMPLE - Floyd's algorithm over the M = nb_houses - 1 others of receiver r, other index o standing
 * for house o if o < r and o + 1 otherwise: for j = M - c .. M - 1 in this order, t = (word_j * (j + 1)) >> 32 in 64-bit arithmetic;
 * t is taken unless it already was, then j is.  word_j = word (j & 3) of Philox4x32-10 with key = seed and counter
 *   (a low word,  a >> 32 | (j >> 2) << 16 | hop << 29 | 1 << 31,  step low word + *step_dev,  0x544D4732 ^ step high word),
 * a the RECEIVER's agent index in the whole batch (below 2^48; -4 beyond).  Bit 31 of the second word is never set in the counters of
 * the action draw (mdr_actor_sample) and of the dead-sender draw (mdr_tarmac_comm), whose second word is a >> 32 < 2^16, and the
 * fourth word's tag differs from theirs: the three streams are disjoint for every (agent, step, hop).  The draw depends on (seed,
 * step + *step_dev, hop, agent) alone - not on the grid, the tiling or the number of envs - and c = nb_houses - 1 gives every other
 * agent.  The reference draws ONE mask per forward call with np.random and shares it among the envs of the batch; here every env
 * (every receiver) has its own draw, as every env has its own dead senders in mdr_tarmac_comm.
 * Further limits (-4): c <= 64 in MDR_TARMAC_RANDOM_SAMPLE; all nb_houses key | value rows of an env are staged in the 160 KB of LDS
 * of a workgroup at a stride of K + V floats rounded up to an odd multiple of 4, beside 512 * c bytes of index lists in
 * MDR_TARMAC_RANDOM_SAMPLE (K = 8, V = 16: nb_houses <= 1462, or 1417 at c = 10).  Every element of every out row is written, no
 * column beyond num_value is; a refused call launches nothing and writes nothing.  An unknown mode is -1. */
int mdr_tarmac_gather(const float *query, int64_t ldq, const float *key, int64_t ldk, const float *value, int64_t ldv, int32_t nb_envs,
                      int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode, uint64_t seed,
                      uint64_t step, const int32_t *step_dev, int32_t hop, float *out, int64_t ldo, void *stream);

/* Its gradient: the formulas and the operand conventions of mdr_tarmac_comm_backward with S(r) the sender sets above, redrawn from the
 * same (seed, step, *step_dev, hop) - no mask is stored between forward and backward.  Two passes, no floating-point atomics: per
 * receiver the statistics and grad_query (MDR_TARMAC_RANDOM_SAMPLE: and the receiver's index list, left in the workspace), then per
 * sender, which scans the receivers of its env in ascending order - the same operands give the same bits.  Covers nb_houses <= 256
 * (whole envs per workgroup; the training minibatches are envs of tens of agents), -4 beyond.  `workspace`: 16-byte aligned device
 * memory of mdr_tarmac_gather_backward_workspace_bytes() bytes, always required. */
int mdr_tarmac_gather_backward(const float *query, int64_t ldq, const float *key, int64_t ldk, const float *value, int64_t ldv,
                               int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value, int32_t nb_comm, int32_t mode,
                               uint64_t seed, uint64_t step, const int32_t *step_dev, int32_t hop, const float *out, int64_t ldo,
                               const float *grad_out, int64_t ldg, float *grad_query, int64_t ldgq, float *grad_key, int64_t ldgk,
                               float *grad_value, int64_t ldgv, void *workspace, void *stream);

/* 16 bytes of statistics per agent, plus in MDR_TARMAC_RANDOM_SAMPLE 2 c bytes per agent rounded up to 16 in all
 * (c = min(nb_comm, nb_houses - 1)); -1 for sizes or a mode the calls refuse. */
int64_t mdr_tarmac_gather_backward_workspace_bytes(int32_t nb_envs, int32_t nb_houses, int32_t num_key, int32_t num_value,
                                                   int32_t nb_comm, int32_t mode);

/* The policy head's last step for two logits per agent (`logits` float [nb_agents][ld], ld >= 2, columns 0 and 1):
 * d = l0 - l1, p0 = 1 / (1 + exp(-d)), p1 = 1 / (1 + exp(d)), then the draw, `action`, `a_prob`, `probs` and `step_dev` exactly as
 * mdr_actor_sample: for equal probabilities the same (seed, step, agent) draws the same action.  greedy != 0: argmax, the first
 * maximum on ties, no draw. */
int mdr_logits_sample(const float *logits, int64_t ld, int64_t nb_agents, uint64_t seed, uint64_t step, const int32_t *step_dev,
                      int32_t greedy, uint8_t *action, float *a_prob, float *probs, void *stream);

/* ---- The whole TarMAC actor through the C ABI: its per-agent MLPs on the matrix cores - exact fp32 on v_mfma_f32_16x16x4_f32 with
 * 16 agents per wavefront (csrc/mdr_tarmac_mlp.hip), or bf16x3 on v_mfma_f32_16x16x32_bf16 with 32 (csrc/mdr_tarmac_mlp_bf16.hip), see
 * mdr_tarmac_precision - and the attention through the kernel behind the attention entry point above, in fp32, once per hop.
 *
 * Notation: F = num_state, H = hidden, K = num_key, V = num_value, M = H + V; nb(n) = ceil(n / 16) blocks of 16 units, nbH = nb(H),
 * nbV = nb(V), nbM = nb(M); lane = 0..63, r = lane & 15, g = lane >> 4.  Wz is a torch weight matrix [out][in] zero-padded to whole
 * blocks of rows and to the columns a fragment asks for.  A FRAGMENT of a layer with S k-steps and nbO output blocks holds, for
 * k-step s, the lane's weight for every output block, the blocks in chunks of four - chunk j holds w_j = min(4, nbO - 4 j) blocks:
 *   frag[s][j][lane][i < w_j] = Wz[16 (4 j + i) + r][col(s, g)]          (64 nbO floats per k-step, chunk j starts 256 j floats in)
 * with col(s, g) one of
 *   rows(S, c0): c0 + g S + s          the input is read from memory, lane group g holding S consecutive floats of its agent's row
 *   regs:        16 (s >> 2) + 4 g + (s & 3)   the input is the previous layer's accumulator (S = 4 x that layer's blocks)
 *
 *   frag_encode = obs2hidden.0  rows(ceil(F / 4), 0), nbH blocks  |  obs2hidden.2  regs (4 nbH steps), nbH blocks
 *   frag_proj   = hidden2query.0 | hidden2key.0 | hidden2value.0  each regs (4 nbH), nbH blocks
 *               | hidden2query.2  regs (4 nbH), 1 block | hidden2key.2  regs (4 nbH), 1 block | hidden2value.2  regs (4 nbH), nbV blocks
 *   frag_msg    = msg_state2state.0: V / 4 steps rows(V / 4, 0) - the comm columns of the concatenation [comm, h] - then H / 4 steps
 *                 rows(H / 4, V), nbM blocks  |  msg_state2state.2  regs (4 nbM), nbH blocks
 *   frag_head   = comm_hidden2action.0  rows(M / 4, 0), nbH blocks - the row [x, comm]; without communication hidden2action.0
 *                 rows(H / 4, 0)
 *   vec         = every bias zero-padded to whole blocks, in unit order, then the head:
 *                 obs2hidden.0 [16 nbH] | obs2hidden.2 [16 nbH] | hidden2query.0 | hidden2key.0 | hidden2value.0 [16 nbH each]
 *                 | hidden2query.2 [16] | hidden2key.2 [16] | hidden2value.2 [16 nbV] | msg_state2state.0 [16 nbM] | msg_state2state.2 [16 nbH]
 *                 | head.0 [16 nbH] | W3[0][u] - W3[1][u], u < 16 nbH | b3[0] - b3[1], 0, 0, 0      (W3, b3: the head's last layer)
 * Parts an actor does not have (no communication: frag_proj, frag_msg; one hop: frag_msg) may be NULL; their slots in vec are zeros.
 * All five pointers are device memory, 16-byte aligned.
 *
 * precision = MDR_TARMAC_BF16X3: vec is unchanged (fp32); the four frag_* arrays hold the same layers in the same sequence as bf16
 * head / tail fragments of 8 bf16 (4-byte words, as mdr_actor_t's MDR_ACTOR_BF16X3).  A layer with S k-steps and nbO output blocks is
 *   frag[s][mb < nbO][t][lane][j < 8] = split_t(Wz[16 mb + r][col(s, g, j)]),  t = 0 head / 1 tail     (512 words per (s, mb) pair)
 * split_0(w) = bf16(w), split_1(w) = bf16(w - split_0(w)), round to nearest even; bf16 j of a lane in the low (even j) / high (odd j)
 * half of word j / 2; a k-step covers 32 inputs, col(s, g, j) one of
 *   rows(n, c0): c0 + 32 s + 8 g + j     S = ceil(n / 32): the input is n consecutive floats of the agent's row; zero where 32 s + 8 g + j >= n
 *   regs(nbI):   16 (2 s + (j >> 2)) + 4 g + (j & 3)     S = ceil(nbI / 2): the input is the previous layer's accumulator of nbI blocks;
 *                zero where 2 s + (j >> 2) >= nbI (the unused half of an odd last k-step) and past the layer's inputs
 *   frag_encode = obs2hidden.0  rows(F, 0), nbH blocks  |  obs2hidden.2  regs(nbH), nbH blocks
 *   frag_proj   = hidden2query.0 | hidden2key.0 | hidden2value.0  each regs(nbH), nbH blocks
 *               | hidden2query.2  regs(nbH), 1 block | hidden2key.2  regs(nbH), 1 block | hidden2value.2  regs(nbH), nbV blocks
 *   frag_msg    = msg_state2state.0: the k-steps rows(V, 0) - the comm columns - then, in k-steps of their own, rows(H, V), nbM blocks
 *               | msg_state2state.2  regs(nbM), nbH blocks
 *   frag_head   = comm_hidden2action.0  rows(M, 0), nbH blocks; without communication hidden2action.0  rows(H, 0) */
typedef struct mdr_tarmac_actor {
  uint32_t struct_size;
  int32_t num_state;   /* F <= 64 */
  int32_t hidden;      /* H: a multiple of 4, <= 64 */
  int32_t num_key;     /* K: a multiple of 4, <= 16 */
  int32_t num_value;   /* V: a multiple of 4, <= 32 */
  int32_t nb_comm;     /* number_agents_comm before the clamp to nb_houses - 1; <= 64 after it */
  int32_t mode;        /* mdr_tarmac_mode */
  int32_t num_hops;    /* 1..4 */
  int32_t with_comm;   /* 0: obs2hidden -> hidden2action, no attention */
  float defect_prob;   /* comm_defect_prob, drawn as the attention entry point documents */
  int32_t greedy;      /* argmax, the first maximum on ties, no draw */
  int32_t precision;   /* mdr_tarmac_precision; 0 (a zeroed field) = MDR_TARMAC_FP32.  Any other value: -1 from mdr_tarmac_actor_sample */
  const float *frag_encode;
  const float *frag_proj;
  const float *frag_msg;
  const float *frag_head;
  const float *vec;
} mdr_tarmac_actor_t;

/* Sizes in floats of the five arrays (-1: a shape no fragment exists for) */
int64_t mdr_tarmac_frag_encode_floats(int32_t num_state, int32_t hidden);
int64_t mdr_tarmac_frag_proj_floats(int32_t hidden, int32_t num_value);
int64_t mdr_tarmac_frag_msg_floats(int32_t hidden, int32_t num_value);
int64_t mdr_tarmac_frag_head_floats(int32_t hidden, int32_t num_value, int32_t with_comm);
int64_t mdr_tarmac_vec_floats(int32_t hidden, int32_t num_value);
/* Size in 4-byte words of frag_encode (part 0), frag_proj (1), frag_msg (2) or frag_head (3) for the struct's shape, with_comm and
 * precision (reads those fields only; host-only, no device call): with MDR_TARMAC_FP32 what the four helpers above return.  -1: a
 * shape outside the struct's limits, another part or precision, a struct_size that is not this header's. */
int64_t mdr_tarmac_frag_words(const mdr_tarmac_actor_t *actor, int32_t part);
/* Bytes of device scratch a sample of nb_agents = nb_envs * nb_houses agents needs (reads the shape fields only): the head's input
 * [A][H + V], the packed projections [A][K + K + V] and, with more than one hop, the state [A][H]. */
int64_t mdr_tarmac_actor_workspace_bytes(const mdr_tarmac_actor_t *actor, int64_t nb_agents);

/* TarmacPPO.select_actions (agents/tarmac_ppo.py:83-95) for every env at once: `obs` float rows [nb_envs * nb_houses][F] ->
 * `action` uint8 [A], `a_prob` float [A] (may be NULL), `probs` float [A][2] (may be NULL).  Enqueues 1 + hops + (hops - 1) + 1
 * kernels on `stream` (two without communication) and never synchronises or allocates; `workspace`: 16-byte aligned device memory
 * of the size above, owned by the caller, its contents free between calls.  The attention, its defect draws, the action draw,
 * `step_dev` and greedy are those of the two entry points above for the same (seed, step, agent), in either precision: the action is the
 * draw compared with the kernel's own probs[0].  Returns 0, -1 (invalid argument:
 * a NULL or misaligned pointer, a struct_size that is not this header's, a precision that is neither of the two), -3 (HIP error) or -4 (a shape outside the limits in the
 * struct above, or c > 64 after the clamp); on -1 and -4 nothing was launched and no output touched. */
int mdr_tarmac_actor_sample(const mdr_tarmac_actor_t *actor, const float *obs, int32_t nb_envs, int32_t nb_houses, uint64_t seed,
                            uint64_t step, const int32_t *step_dev, void *workspace, uint8_t *action, float *a_prob, float *probs,
                            void *stream);

/* Observe -> act for the TarMAC actor: mdr_tarmac_actor_sample on the observation of every agent of `env` in its current state,
 * WITHOUT the observation rows.  The first kernel of the chain builds the 51 normStateDict features of its tile of agents in LDS from
 * the compact state - the staging of mdr_env_actor_sample - and reads its layer-1 operands from there in the k-step order of
 * frag_encode: the same fragments serve both entry points, and `action`, `a_prob` and `probs` are bit for bit those of
 * mdr_tarmac_actor_sample on the rows of mdr_env_obs_vector(MDR_OBS_ROWS) for the same (seed, step, *step_dev), in either precision
 * (agent index = env * nb_houses + house).  `workspace` (mdr_tarmac_actor_workspace_bytes), `step_dev` and capture in a graph as
 * there.  `rows_out` as mdr_env_actor_sample (may be NULL): the rows float [nb_agents][51], bit for bit those of mdr_env_obs_vector.
 * Covers what the default form of mdr_env_actor_sample covers - every optional state / message column off, agents_comm_mode
 * "neighbours" with nb_agents_comm = 10, no link defects, unsharded houses, nb_houses >= 11 - and actor->num_state = 51; the actor's
 * own nb_comm, mode, defect_prob and num_hops are the attention's and unrelated to the env's message senders: every value
 * mdr_tarmac_actor_sample takes is taken.  Anything else returns MDR_ERR_UNSUPPORTED (-4) with nothing launched and nothing
 * written: fall back to mdr_env_obs_vector + mdr_tarmac_actor_sample.  -1 / -3 as mdr_tarmac_actor_sample. */
int mdr_env_tarmac_actor_sample(mdr_env_t *env, const mdr_obs_spec_t *spec, const mdr_tarmac_actor_t *actor, uint64_t seed, uint64_t step,
                                const int32_t *step_dev, void *workspace, uint8_t *action, float *a_prob, float *probs, float *rows_out,
                                void *stream);

/* ---- PPO's update step for the MLP actor and critic (PPO.update, agents/ppo.py:139-188): loss and gradient of one minibatch.
 *
 * One network of agents/network.py:14-57 - Linear(F,H1) - ReLU - Linear(H1,H2) - ReLU - Linear(H2,O) - in torch's own layout,
 * w[out][in] contiguous, device memory, read as it is on every call (an optimiser step changes it between any two calls: there is
 * nothing to repack).  Limits: F <= 64, H1 <= 128, H2 <= 128, O = 2 (actor) or 1 (critic).  The observations with message columns
 * (81, 91, 121 features) are outside them and go to the mdr_*_wide entry points behind the DQN block below: F <= 128 and the LDS fit
 * (hidden 100-100 at every F <= 128; 128-128 up to F = 100).  MAPPO's critic on state + others' actions has an entry point of its
 * own with a wider input (mdr_mappo_critic_grad below: up to 128 joint features). */
typedef struct mdr_mlp {
  uint32_t struct_size;
  int32_t num_state, hidden1, hidden2, num_out;
  const float *w1, *b1, *w2, *b2, *w3, *b3;
} mdr_mlp_t;

/* Floats of the flat gradient dW1 [H1][F] | db1 [H1] | dW2 [H2][H1] | db2 [H2] | dW3 [O][H2] | db3 [O] - torch's parameter order and
 * layout (reads the shape fields only; host-only, no device call).  -1: a shape outside the limits, a struct_size that is not this
 * header's. */
int64_t mdr_mlp_grad_floats(const mdr_mlp_t *net);
/* Bytes of device scratch one gradient call over nb_rows minibatch rows with this max_workgroups needs: one partial gradient per
 * workgroup (host-only, no device call; with max_workgroups = 0 enough for the library's own grid on any device).  -1 as above, or
 * nb_rows < 0, max_workgroups < 0. */
int64_t mdr_mlp_grad_workspace_bytes(const mdr_mlp_t *net, int64_t nb_rows, int32_t max_workgroups);

/* The clipped surrogate of agents/ppo.py:153-166 and its gradient.  Minibatch row i < nb_rows is transition j = index ? index[i] : i
 * (`index` device int64, may be NULL: BatchSampler's indices into the buffer); `state` + j * ld_state its F floats (ld_state >= F),
 * `action[j]` (int64, nonzero = action 1), `old_prob[j]` the stored probability of the taken action - whole-buffer arrays read through
 * `index` -, `advantage[i]` in minibatch order.  p = softmax(actor(state_j)), ratio_i = p[action_j] / old_prob_j,
 *   loss = -(1 / nb_rows) sum_i min(ratio_i A_i, clamp(ratio_i, 1 - clip_param, 1 + clip_param) A_i)
 * and `grad` (mdr_mlp_grad_floats floats) = d loss / d parameters as torch's autograd takes it: d loss / d ratio_i = -A_i / nb_rows
 * where 1 - clip <= ratio_i <= 1 + clip (bounds included) or ratio_i A_i < clamp(ratio_i) A_i, else 0; relu'(z) = 1 iff z > 0.
 * old_prob = 0 gives inf / NaN as in the reference.  `loss`: one float on the device.  `ratio` (may be NULL): float [nb_rows].
 * Exact fp32 on the matrix cores; a persistent grid of min(tiles of 16 rows, max_workgroups) workgroups (0: the library's choice,
 * min(tiles, compute units, 512)) each leaves one partial gradient in `workspace`, a second launch adds them in workgroup order and
 * divides by nb_rows: no floating-point atomics, the same inputs and the same max_workgroups give the same bits on every call.
 * Every float of `grad`, `loss` and `ratio` is written by every successful call; nb_rows == 0 writes zeros to `grad` and `loss`.
 * Stream-ordered, never synchronises, allocates nothing; `workspace`: 16-byte aligned device memory of
 * mdr_mlp_grad_workspace_bytes, owned by the caller, its contents free before and after the call.
 * Returns 0; -1 (a NULL required pointer, ld_state < F, nb_rows < 0, max_workgroups < 0, clip_param outside [0, 1), a struct_size
 * that is not this header's, a missing or misaligned workspace); -3 (HIP error); -4 (a shape outside the limits, num_out != 2).  On
 * -1 and -4 nothing was launched and nothing written. */
int mdr_ppo_actor_grad(const mdr_mlp_t *actor, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                       const int64_t *action, const float *old_prob, const float *advantage, float clip_param,
                       int32_t max_workgroups, void *workspace, float *grad, float *loss, float *ratio, void *stream);

/* The value loss of agents/ppo.py:149-150, 173: V_i = critic(state_j), loss = (1 / nb_rows) sum_i (target_j - V_i)^2 (F.mse_loss),
 * `target` a whole-buffer array read through `index`.  `value` (may be NULL): V_i; `advantage` (may be NULL): target_j - V_i, the
 * detached delta mdr_ppo_actor_grad takes; both float [nb_rows] in minibatch order.  Everything else - rows, `grad`, `loss`,
 * workspace, grid, determinism, return codes (-4: num_out != 1) - as mdr_ppo_actor_grad. */
int mdr_ppo_critic_grad(const mdr_mlp_t *critic, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                        const float *target, int32_t max_workgroups, void *workspace, float *grad, float *loss, float *value,
                        float *advantage, void *stream);

/* The bf16x3 precision of the two calls above: the argument lists, the limits, the flat gradient, the workspace
 * (mdr_mlp_grad_floats, mdr_mlp_grad_workspace_bytes: the same grid of 16-row tiles), the determinism and the return codes of
 * mdr_ppo_actor_grad / mdr_ppo_critic_grad, with the five matrix products on v_mfma_f32_16x16x32_bf16.  The contract:
 *   F1 (W1 x), F2 (W2 h1), B2 (W2^T dz2), dW2 = dz2^T h1 and dW1 = dz1^T x take every operand split a = ah + al, ah = bf16(a),
 *   al = bf16(a - ah), round to nearest even, and every product as ah bh + al bh + ah bl, accumulated in fp32 (the al bl term is
 *   dropped: a product of two operands that do not split exactly is off by up to 2^-15 |a| |b|, operands that are exact in bf16
 *   or split exactly lose nothing);
 *   everything else is fp32 as in the calls above: biases, ReLU, the logits and dW3 / db3, the head's loss and dlogits, relu'(z) =
 *   [z > 0] on the call's own z, the bias gradients, rows past the minibatch adding exact zeros.
 * The weights are read in place and split on every call: nothing is packed, the next call sees an optimiser step.  Every shape
 * inside the limits (F <= 64, H1, H2 <= 128) is taken; -4: a shape outside them, num_out != 2 (actor) / 1 (critic).  On -1 and -4
 * nothing was launched and nothing written. */
int mdr_ppo_actor_grad_bf16x3(const mdr_mlp_t *actor, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                              const int64_t *action, const float *old_prob, const float *advantage, float clip_param,
                              int32_t max_workgroups, void *workspace, float *grad, float *loss, float *ratio, void *stream);
int mdr_ppo_critic_grad_bf16x3(const mdr_mlp_t *critic, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                               const float *target, int32_t max_workgroups, void *workspace, float *grad, float *loss, float *value,
                               float *advantage, void *stream);

/* ---- MAPPO's update step (MAPPO.update, agents/mappo.py:60-119).  Its actor step is PPO's line for line (mappo.py:92-110 against
 * ppo.py:153-169): mdr_ppo_actor_grad serves it.  Its critic is Critic(num_state + nb_agents - 1) on torch.cat((state, others_actions))
 * (mappo.py:21, 87): an mdr_mlp_t with num_state = J = F + (nb_agents - 1) and num_out = 1, parameters in torch's own layout.
 *
 * Floats of the joint critic's flat gradient dW1 [H1][J] | db1 [H1] | dW2 [H2][H1] | db2 [H2] | dW3 [1][H2] | db3 [1] (host-only, no
 * device call).  -1: nb_agents < 1, J - (nb_agents - 1) < 1, num_out != 1, J > 128, a hidden layer > 128, a shape whose LDS layout does
 * not fit (hidden 100-100 fits up to J = 100, 128-128 up to J = 68, 64-64 at J = 128), a struct_size that is not this header's. */
int64_t mdr_mappo_critic_grad_floats(const mdr_mlp_t *critic, int32_t nb_agents);
/* Bytes of device scratch one mdr_mappo_critic_grad call needs, as mdr_mlp_grad_workspace_bytes (host-only).  -1 as above, or
 * nb_rows < 0, max_workgroups < 0. */
int64_t mdr_mappo_critic_workspace_bytes(const mdr_mlp_t *critic, int32_t nb_agents, int64_t nb_rows, int32_t max_workgroups);

/* The value loss of agents/mappo.py:85-88, 113 and its gradient.  Minibatch row i < nb_rows is transition j = index ? index[i] : i of
 * a buffer of nb_transitions transitions in collect_ppo_rollout's flat layout: the agent index runs fastest, so transition j is agent
 * a = j % nb_agents and its env-mates are the nb_agents transitions from j - a on (nb_transitions a multiple of nb_agents).  The
 * critic's input is the F = J - (nb_agents - 1) floats at `state` + j * ld_state (ld_state >= F) followed by the others' actions,
 *   input[F + k] = action[j - a + k + (k >= a)] != 0 ? 1 : 0,   k < nb_agents - 1
 * (train_mappo.py:79-84: the step's action dict without agent a, in agent order), gathered from the whole-buffer `action` (int64
 * [nb_transitions]) while the tile is staged: no others_actions tensor is read or needed.  V_i = critic(input_i),
 *   loss = (1 / nb_rows) sum_i (target_j - V_i)^2
 * and `grad` (mdr_mappo_critic_grad_floats floats) = d loss / d parameters as torch's autograd takes it; `target` a whole-buffer array
 * read through `index`; `value` (may be NULL): V_i; `advantage` (may be NULL): target_j - V_i; both float [nb_rows] in minibatch
 * order.  Every element of `grad`, `loss` and the given `value` / `advantage` is written by every successful call; nb_rows == 0 writes
 * zeros to `grad` and `loss`.  Exact fp32 on the matrix cores, grid, partials in `workspace` (mdr_mappo_critic_workspace_bytes, 16-byte
 * aligned), determinism (no floating-point atomics) and the stream contract as mdr_ppo_critic_grad.
 * Returns 0; -1 (a NULL required pointer, nb_agents < 1, critic->num_state - (nb_agents - 1) < 1, ld_state < F, nb_transitions not a
 * multiple of nb_agents, nb_rows < 0, max_workgroups < 0, a struct_size that is not this header's, a missing or misaligned
 * workspace); -3 (HIP error); -4 (num_out != 1, J > 128, a hidden layer > 128, an LDS layout that does not fit).  On -1 and -4
 * nothing was launched and nothing written. */
int mdr_mappo_critic_grad(const mdr_mlp_t *critic, const float *state, int64_t ld_state, const int64_t *action, int64_t nb_transitions,
                          int32_t nb_agents, const int64_t *index, int64_t nb_rows, const float *target, int32_t max_workgroups,
                          void *workspace, float *grad, float *loss, float *value, float *advantage, void *stream);

/* ---- DQN's / DDQN's update step on the same network (DQN.update, agents/dqn.py:84-112; DDQN.update, :119-146): the TD target of a
 * minibatch, then the Huber loss and its clamped gradient.  Both nets are DQN_network (agents/network.py:58-77, raw Q-values) as
 * mdr_mlp_t with num_out = 2 and the limits above.
 *
 * The TD target.  Minibatch row i < nb_rows is transition j = index ? index[i] : i (`index` device int64, may be NULL: the replay
 * buffer's sampled positions); `next_state` + j * ld_state its F floats (ld_state >= F) and `reward[j]` - whole-buffer arrays read
 * through `index`.  With (Q0, Q1) = target_net(next_state_j):
 *   policy_net == NULL (DQN, dqn.py:96):   next_q[i] = max(Q0, Q1), next_action[i] (when given) = Q1 > Q0, the target net's own argmax
 *   policy_net != NULL (DDQN, dqn.py:129-132): next_action[i] = argmax policy_net(next_state_j), next_q[i] = Q[next_action[i]]
 *   y[i] = reward[j] + gamma * next_q[i]   (dqn.py:99; the product and the sum each rounded to fp32, no fma)
 * A tie gives action 0, the first maximal index, as torch.argmax does; a NaN Q1 is taken as the maximum (torch.max).  There is no
 * terminal mask: the reference's env never ends.  The reference's DDQN adds reward [B, 1] to next_q [B, 1, 1] and so broadcasts the
 * target to [B, B, 1] (dqn.py:132-135); this is the per-row target that line evidently means.  `y`, `next_q` (may be NULL): float
 * [nb_rows]; `next_action`: uint8 [nb_rows], required for DDQN, else may be NULL; all in minibatch order.
 * Forward only, exact fp32 on the matrix cores: the gradient kernels' staging, two hidden layers and logits on a persistent grid of
 * min(tiles of 16 rows, max_workgroups) workgroups (0: the library's choice, min(tiles, compute units, 512)), nothing else - no
 * workspace.  DDQN makes two such launches, policy_net first (it writes next_action), target_net second (it reads it): the two weight
 * sets do not fit the 160 KB of LDS together.  Every element of every given output is written by every successful call; nb_rows == 0
 * launches nothing.  The same inputs give the same bits on every call.  Stream-ordered, never synchronises, allocates nothing.
 * Returns 0; -1 (a NULL required pointer - DDQN without next_action included -, ld_state < F, nb_rows < 0, max_workgroups < 0, gamma
 * not finite, a struct_size that is not this header's); -3 (HIP error); -4 (a shape outside the limits, num_out != 2, for DDQN two
 * nets of different shapes).  On -1 and -4 nothing was launched and nothing written. */
int mdr_dqn_target(const mdr_mlp_t *target_net, const mdr_mlp_t *policy_net, const float *next_state, int64_t ld_state,
                   const int64_t *index, int64_t nb_rows, const float *reward, float gamma, int32_t max_workgroups, float *y,
                   float *next_q, uint8_t *next_action, void *stream);

/* nn.SmoothL1Loss() of dqn.py:93, 102-109 and its gradient.  Rows, `state`, `index` as above; `action[j]` (int64, nonzero = action 1) a
 * whole-buffer array read through `index`, `y[i]` (mdr_dqn_target's, detached) in minibatch order.  q_i = policy_net(state_j)[action_j],
 * delta_i = q_i - y_i,
 *   loss = (1 / nb_rows) sum_i (|delta_i| < 1 ? delta_i^2 / 2 : |delta_i| - 1 / 2)
 * and `grad` (mdr_mlp_grad_floats floats) = d loss / d parameters as torch's autograd takes it - d loss / d q_i = (delta_i < -1 ? -1 :
 * delta_i > 1 ? 1 : delta_i) / nb_rows, the other Q-value's gradient 0, relu'(z) = 1 iff z > 0 - with every element then clamped to
 * [-grad_clamp, grad_clamp] (param.grad.data.clamp_(-1, 1)): v < -c ? -c : v > c ? c : v, so a NaN stays a NaN as under clamp_;
 * INFINITY clamps nothing.  The clamp is part of the reduction launch and never touches `loss`.  `q` (may be NULL): float [nb_rows],
 * q_i.  Everything else - `grad`, `loss`, workspace (mdr_mlp_grad_workspace_bytes), grid, determinism, zero rows - as
 * mdr_ppo_actor_grad.  Returns 0; -1 (a NULL required pointer, ld_state < F, nb_rows < 0, max_workgroups < 0, grad_clamp NaN or <= 0,
 * a struct_size that is not this header's, a missing or misaligned workspace); -3 (HIP error); -4 (a shape outside the limits,
 * num_out != 2).  On -1 and -4 nothing was launched and nothing written. */
int mdr_dqn_grad(const mdr_mlp_t *policy_net, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                 const int64_t *action, const float *y, float grad_clamp, int32_t max_workgroups, void *workspace, float *grad,
                 float *loss, float *q, void *stream);

/* ---- The same update steps for 65..128 input features: the observations with message_properties["thermal"] (81 features), ["hvac"]
 * (91) or both (121).  Every entry point above keeps its limits; each has a sibling here with the same argument list, the same
 * arithmetic, the same status codes and the same contract (checks on the host before any launch, nothing written on -1 and -4).
 * Limits: F <= 128 (the joint critic: J <= 128), H1 <= 128, H2 <= 128 and the LDS fit.  From F = 65 on they run an instantiation of
 * the kernel with 8 dW1 blocks per wave and an LDS layout in which the image of dz1 shares the storage of h2 (the two are never live
 * at once), which fits
 *   hidden 100-100 (.. 112-112) at every F <= 128,   128-128 up to F = 100,   64-64 .. 96-96 at every F <= 128;
 * a shape that does not fit - 128-128 at F = 101 - returns -4 (the size queries -1).  For F <= 64 a wide entry point is its narrow
 * sibling: the same kernel, the same bits.  mdr_mappo_critic_grad_wide takes the same kernel as mdr_mappo_critic_grad with the shared
 * image, so 100-100 fits up to J = 128 (above: 100) and 128-128 up to J = 100 (above: 68); it returns mdr_mappo_critic_grad's bits
 * wherever both accept.  J > 128 - F = 121 with 20 agents is J = 140 - stays refused.
 * mdr_dqn_target_wide refuses what mdr_dqn_grad_wide refuses (its own forward-only image would fit a little more): the pair is
 * accepted or refused together.  Sizes: mdr_mlp_wide_grad_floats / mdr_mlp_wide_grad_workspace_bytes for the actor, critic and DQN
 * calls (equal to the narrow queries wherever those answer), mdr_mappo_critic_wide_grad_floats / _wide_workspace_bytes for the joint
 * critic. */
int64_t mdr_mlp_wide_grad_floats(const mdr_mlp_t *net);
int64_t mdr_mlp_wide_grad_workspace_bytes(const mdr_mlp_t *net, int64_t nb_rows, int32_t max_workgroups);
int mdr_ppo_actor_grad_wide(const mdr_mlp_t *actor, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                            const int64_t *action, const float *old_prob, const float *advantage, float clip_param,
                            int32_t max_workgroups, void *workspace, float *grad, float *loss, float *ratio, void *stream);
int mdr_ppo_critic_grad_wide(const mdr_mlp_t *critic, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                             const float *target, int32_t max_workgroups, void *workspace, float *grad, float *loss, float *value,
                             float *advantage, void *stream);
int mdr_dqn_target_wide(const mdr_mlp_t *target_net, const mdr_mlp_t *policy_net, const float *next_state, int64_t ld_state,
                        const int64_t *index, int64_t nb_rows, const float *reward, float gamma, int32_t max_workgroups, float *y,
                        float *next_q, uint8_t *next_action, void *stream);
int mdr_dqn_grad_wide(const mdr_mlp_t *policy_net, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                      const int64_t *action, const float *y, float grad_clamp, int32_t max_workgroups, void *workspace, float *grad,
                      float *loss, float *q, void *stream);
int64_t mdr_mappo_critic_wide_grad_floats(const mdr_mlp_t *critic, int32_t nb_agents);
int64_t mdr_mappo_critic_wide_workspace_bytes(const mdr_mlp_t *critic, int32_t nb_agents, int64_t nb_rows, int32_t max_workgroups);
int mdr_mappo_critic_grad_wide(const mdr_mlp_t *critic, const float *state, int64_t ld_state, const int64_t *action,
                               int64_t nb_transitions, int32_t nb_agents, const int64_t *index, int64_t nb_rows, const float *target,
                               int32_t max_workgroups, void *workspace, float *grad, float *loss, float *value, float *advantage,
                               void *stream);

/* ---- MADDPG's update step (MADDPG.update, agents/ddpg.py:305-339) with one shared actor, critic and target of each: for agent a the
 * TD target through both target nets, the joint critic's mse loss and gradient, the gumbel-softmax actor's loss and gradient.  All
 * four nets are DDPG_Network (agents/network.py:80-100) as mdr_mlp_t in torch's own layout, read as they are on every call.  The
 * actor: num_state = F <= 64, num_out = 2.  The critic: num_state = J = nb_agents (F + 2) <= 1280, num_out = 1.  Every hidden layer
 * <= 256 units, any size (no multiple of 16 needed): the reference's 20 x (51 + 2) = 1060 inputs with 256-256 hidden units and
 * nb_agents = 1 are inside.  The weights do not fit LDS at these sizes, so this family streams them from L2 (mdr_maddpg_grad.hip) and
 * is separate from the entry points above, whose limits and code are unchanged.
 *
 * Rows.  Minibatch row i < nb_rows is stored env-step j = index ? index[i] : i (`index` device int64, may be NULL).  An env-step
 * holds `state` + j * ld_state: nb_agents F contiguous floats in agent order (ld_state >= nb_agents F); `action[j * nb_agents + k]`
 * (int64, nonzero = action 1); `reward[j * nb_agents + k]`.  The critic's joint input is
 *   x = state_j (nb_agents F floats) | onehot(action[j][0]) | ... | onehot(action[j][nb_agents - 1]),
 * column nb_agents F + 2 k + c = (action[j][k] != 0) == c, gathered while a tile is staged and again by the weight gradient: no joint
 * tensor is read or stored.  Gumbel noise is an input (float32, drawn by the caller as -log(Exp(1))): no kernel draws random numbers.
 * The pick of logits l with noise g: t_c = (l_c + g_c) / tau, action 1 iff t_1 > t_0 (a tie: action 0, as max(dim)[1]); its forward
 * value is the exact one-hot (torch's y_hard - y_soft.detach() + y_soft has the same bits in fp32).
 *
 * Common to the three calls: exact fp32 on v_mfma_f32_16x16x4_f32, no floating-point atomics, the same inputs and the same
 * max_workgroups give the same bits on every call; every element of every given output is written by every successful call.  A row
 * pass (one workgroup of 1024 threads per tile of 16 rows, a persistent grid of min(tiles, max_workgroups) workgroups; 0: the
 * library's choice, min(tiles, compute units, 512)) does everything of a row; the gradient calls follow it with a weight pass, one
 * wave per 16 x 16 block of a weight gradient, summing over the minibatch rows in row order (at most max_workgroups workgroups of
 * four waves; 0: one wave per block).  Stream-ordered, never synchronise, allocate nothing.  There is no terminal mask: the
 * reference's env never ends.
 *
 * Floats of the flat gradient of one net, dW1 | db1 | dW2 | db2 | dW3 | db3 in torch's parameter order and layout (host-only).  -1:
 * num_state > 1280, a hidden layer > 256, num_out not 1 or 2, a struct_size that is not this header's. */
int64_t mdr_maddpg_grad_floats(const mdr_mlp_t *net);
/* Bytes of device scratch mdr_maddpg_critic_grad or mdr_maddpg_actor_grad needs over nb_rows rows (the larger of the two; h1, h2,
 * dz1, dz2 of the differentiated net, dlogits and the rows' loss terms; host-only, independent of max_workgroups).  -1: shapes
 * outside the limits or that do not fit each other (critic->num_state != nb_agents (actor->num_state + 2)), nb_rows < 0,
 * max_workgroups < 0. */
int64_t mdr_maddpg_workspace_bytes(const mdr_mlp_t *actor, const mdr_mlp_t *critic, int32_t nb_agents, int64_t nb_rows,
                                   int32_t max_workgroups);

/* The TD target of agent `agent` (ddpg.py:132-142, 282-284, 317-322).  next_action[i][k] = the pick on tgt_actor(next_state_j's F
 * floats of agent k) with noise[i][k][0..1]; x' = next_state_j | onehot(next_action[i][.]); next_q[i] = tgt_critic(x');
 *   y[i] = reward[j][agent] + gamma * next_q[i]      (the product and the sum each rounded to fp32, no fma)
 * `y` float [nb_rows], `next_q` (may be NULL) float [nb_rows], `next_action` uint8 [nb_rows][nb_agents] (required: the second launch
 * reads what the first wrote).  Two launches: the picks over the nb_rows nb_agents actor rows, then the critic's forward.  No
 * workspace.  nb_rows == 0 launches nothing.
 * Returns 0; -1 (a NULL required pointer, nb_agents < 1, nets that do not fit each other, ld_state < nb_agents F, agent outside
 * [0, nb_agents), nb_rows < 0, max_workgroups < 0, tau <= 0 or not finite, gamma not finite, a struct_size that is not this
 * header's); -3 (HIP error); -4 (a shape outside the limits).  On -1 and -4 nothing was launched and nothing written. */
int mdr_maddpg_target(const mdr_mlp_t *tgt_actor, const mdr_mlp_t *tgt_critic, const float *next_state, int64_t ld_state,
                      const float *reward, const int64_t *index, int64_t nb_rows, int32_t nb_agents, int32_t agent, const float *noise,
                      float tau, float gamma, int32_t max_workgroups, float *y, float *next_q, uint8_t *next_action, void *stream);

/* The critic's step (ddpg.py:312-327): q_i = critic(x_i), loss = (1 / nb_rows) sum_i (q_i - y_i)^2 (F.mse_loss), `grad`
 * (mdr_maddpg_grad_floats(critic) floats) = d loss / d parameters as autograd takes it, relu'(z) = 1 iff z > 0.  `y` float [nb_rows]
 * in minibatch order (mdr_maddpg_target's, detached); `q` (may be NULL) float [nb_rows].  `loss`: one float on the device.
 * `workspace`: 16-byte aligned device memory of mdr_maddpg_workspace_bytes, owned by the caller, its contents free before and after
 * the call.  Two launches: row pass, weight pass.  nb_rows == 0 writes zeros to `grad` and `loss` (the weight pass alone).
 * Returns 0; -1 (a NULL required pointer, nb_agents < 1, critic->num_state not nb_agents (F + 2) with F >= 1, ld_state < nb_agents F,
 * nb_rows < 0, max_workgroups < 0, a struct_size that is not this header's, a missing or misaligned workspace); -3; -4 (a shape
 * outside the limits, num_out != 1).  On -1 and -4 nothing was launched and nothing written. */
int mdr_maddpg_critic_grad(const mdr_mlp_t *critic, const float *state, int64_t ld_state, const int64_t *action, const int64_t *index,
                           int64_t nb_rows, int32_t nb_agents, const float *y, int32_t max_workgroups, void *workspace, float *grad,
                           float *loss, float *q, void *stream);

/* The actor's step for agent a = `agent` (ddpg.py:331-339).  l = actor(state_j's F floats of agent a), t = (l + noise[i][0..1]) / tau,
 * p = softmax(t), h the pick; x_i with columns nb_agents F + 2 a, + 1 replaced by onehot(h); Q_i = critic(x_i);
 *   loss = -(1 / nb_rows) sum_i Q_i + pse (1 / (2 nb_rows)) sum_i (l_0^2 + l_1^2)      (the reference: pse = 1e-3)
 * and `grad` (mdr_maddpg_grad_floats(actor) floats) = d loss / d the ACTOR's parameters through the straight-through estimator: with
 * c_o = d loss / d x_i[nb_agents F + 2 a + o] (the critic's backward down to those two input columns only),
 *   dl_0 = p_0 p_1 (c_0 - c_1) / tau + pse l_0 / nb_rows,   dl_1 = -p_0 p_1 (c_0 - c_1) / tau + pse l_1 / nb_rows.
 * The critic is only read: no gradient of it is written.  `q` (may be NULL) float [nb_rows]: Q_i; `logits` (may be NULL) float
 * [nb_rows][2].  `workspace`, launches (two), zero rows and return codes as mdr_maddpg_critic_grad; -1 also for agent outside
 * [0, nb_agents), tau <= 0 or not finite, pse not finite, nets that do not fit each other; -4 also for actor->num_out != 2. */
int mdr_maddpg_actor_grad(const mdr_mlp_t *actor, const mdr_mlp_t *critic, const float *state, int64_t ld_state, const int64_t *action,
                          const int64_t *index, int64_t nb_rows, int32_t nb_agents, int32_t agent, const float *noise, float tau,
                          float pse, int32_t max_workgroups, void *workspace, float *grad, float *loss, float *q, float *logits,
                          void *stream);

/* ---- Acting with an actor of up to 256 hidden units per layer - MADDPG's (DDPG_prop.actor_hidden_dim = 256; ddpg.py:289-298,
 * train_ddpg.py:95-116), beyond the MDR_ACTOR_MAX_HIDDEN = 127 of mdr_actor_sample - in ONE launch: observation rows -> Linear - ReLU -
 * Linear - ReLU - Linear(2) -> softmax -> draw or argmax, for every agent (csrc/mdr_mlp_actor.hip).
 *
 * `actor` is the learners' mdr_mlp_t: torch's own layout, w[out][in] contiguous, device memory, read as it is on every call - nothing
 * is packed on the host, so an optimiser step between two calls is seen by the next call (train_maddpg changes the actor at every
 * update: the reason not to go through mdr_actor_t's fragment arrays).  Limits: 1 <= num_state = F <= 128 (the 81 / 91 / 121-feature
 * observations are inside), 1 <= hidden1, hidden2 <= 256, any size (no multiple of 16 needed), num_out == 2.
 * `obs`: float rows, agent i at obs + i * ld_obs, ld_obs >= F; 4-byte alignment suffices (a 51-float row is 204 bytes).  `action` uint8
 * [nb_agents], `a_prob` float [nb_agents] (may be NULL), `probs` float [nb_agents][2] (may be NULL).
 * Semantics, word for word mdr_actor_sample's: d = logit0 - logit1, p0 = 1 / (1 + exp(-d)), p1 = 1 / (1 + exp(d)); the draw of
 * csrc/mdr_draw.h with the agent's index in the batch as the counter and *step_dev (device int32, may be NULL) added to the low word
 * of `step`; action = u < p0 ? 0 : 1, a_prob = probs[action].  greedy != 0: d >= 0 ? 0 : 1, no draw.  For equal probabilities
 * mdr_logits_sample and this call pick the same action for the same (seed, step, agent).
 * Exact fp32: products on v_mfma_f32_16x16x4_f32, accumulation in fp32 starting from the bias; the head is one dot product with
 * W3[0] - W3[1] (the difference rounded to fp32) in per-wave partials added in wave order.  No floating-point atomics: an agent's
 * `probs` bits depend on its row and the weights only - not on its position in the batch, on nb_agents or on the grid.
 * Persistent workgroups hold their slabs of W1 and W2 in registers - loaded once per launch - and stride over tiles of 32 agents; the
 * grid is min(tiles, compute units, max_workgroups if > 0).  Stream-ordered, never synchronises, allocates nothing.
 * Returns 0; -1 (NULL `actor`, a NULL weight pointer, NULL `obs` or `action`, nb_agents < 0, max_workgroups < 0, ld_obs < F, a
 * struct_size that is not this header's); -3 (HIP error); -4 (a shape outside the limits).  On -1 and -4 nothing was launched and
 * nothing written.  nb_agents == 0 returns 0 and launches nothing. */
int mdr_mlp_actor_sample(const mdr_mlp_t *actor, const float *obs, int64_t ld_obs, int64_t nb_agents, uint64_t seed, uint64_t step,
                         const int32_t *step_dev, int32_t greedy, int32_t max_workgroups, uint8_t *action, float *a_prob, float *probs,
                         void *stream);

/* mdr_mlp_actor_sample in bf16x3 (csrc/mdr_mlp_actor_bf16.hip): the same call - parameters, limits, outputs, draw, `step_dev`,
 * `greedy`, grid and return codes word for word - with the two hidden layers on v_mfma_f32_16x16x32_bf16.  Every weight and every
 * input of a hidden layer (the observation floats, relu(h1)) is split into a bf16 head and tail, xh = bf16(x), xl = bf16(x - xh),
 * round to nearest even, and every product is wh xh + wl xh + wh xl (the tail x tail product is dropped), accumulated in fp32
 * starting from the fp32 bias.  The weights are read in place and split on every call - nothing is packed or cached - and every
 * activation is split once.  The head (one fp32 dot product with W3[0] - W3[1] in per-wave partials added in wave order), the softmax
 * and the draw are mdr_mlp_actor_sample's, so for equal probabilities both calls pick the same action.  No floating-point atomics: an
 * agent's `probs` bits depend on its row and the weights only - not on its position in the batch, on nb_agents, ld_obs or the grid.
 * Contract: each probability within 2e-3 |p| + 2e-5 of an fp64 forward of the same weights (mean absolute error below 5e-6 on the
 * tested inputs); the split keeps 2^-16 of every product on top of the fp32 accumulation.  It is NOT the bits of mdr_mlp_actor_sample.
 * On -1 and -4 nothing was launched and nothing written.  nb_agents == 0 returns 0 and launches nothing. */
int mdr_mlp_actor_sample_bf16x3(const mdr_mlp_t *actor, const float *obs, int64_t ld_obs, int64_t nb_agents, uint64_t seed, uint64_t step,
                                const int32_t *step_dev, int32_t greedy, int32_t max_workgroups, uint8_t *action, float *a_prob,
                                float *probs, void *stream);

/* Observe -> act for this actor: mdr_mlp_actor_sample / mdr_mlp_actor_sample_bf16x3 on the observation of every agent of `env` in its
 * current state, WITHOUT the observation rows (csrc/mdr_mlp_actor_observe.hip).  Per tile of 32 agents one wavefront of the workgroup
 * builds the 51 normStateDict features in LDS from the compact state - the staging of mdr_env_actor_sample and
 * mdr_env_tarmac_actor_sample - and the workgroup copies them, feature by feature in torch's order, into the LDS image the rows
 * kernel stages; both layers, the head, the softmax and the draw are that kernel's.  `action`, `a_prob` and `probs` are bit for bit
 * those of mdr_mlp_actor_sample (_bf16x3: of mdr_mlp_actor_sample_bf16x3) on the rows of mdr_env_obs_vector(MDR_OBS_ROWS) with
 * ld_obs = 51 for the same (seed, step, *step_dev, greedy), whatever max_workgroups (agent index = env * nb_houses + house).
 * `rows_out` (may be NULL): float [nb_agents][51], 4-byte aligned, receives the rows as a by-product, bit for bit those of
 * mdr_env_obs_vector.  `actor`, `step_dev`, `greedy`, `max_workgroups`, the grid and capture in a graph as mdr_mlp_actor_sample; the
 * env is only read.  One launch on `stream`, no synchronisation, no allocation.
 * Covers what mdr_env_tarmac_actor_sample covers - every optional state / message column off, agents_comm_mode "neighbours" with
 * nb_agents_comm = 10, no link table, no link defects, unsharded houses, nb_houses >= 11 (the tiles of 32 agents of every cluster
 * size up to 1999 fit the 64 staging lanes; the library checks it for the size it is given) - and actor->num_state == 51, hidden1 and
 * hidden2 anything in 1 .. 256, num_out == 2.  Anything else returns MDR_ERR_UNSUPPORTED (-4) with mdr_last_error set: fall back to
 * mdr_env_obs_vector + mdr_mlp_actor_sample.  -1: NULL `env`, `spec`, `actor` or `action`, a NULL weight pointer, a struct_size that
 * is not this header's, max_workgroups < 0.  Every refusal is decided before anything touches the device: nothing is launched,
 * nothing written.  -3: HIP error.  nb_envs * nb_houses == 0 returns 0 and launches nothing. */
int mdr_env_mlp_actor_sample(mdr_env_t *env, const mdr_obs_spec_t *spec, const mdr_mlp_t *actor, uint64_t seed, uint64_t step,
                             const int32_t *step_dev, int32_t greedy, int32_t max_workgroups, uint8_t *action, float *a_prob, float *probs,
                             float *rows_out, void *stream);
int mdr_env_mlp_actor_sample_bf16x3(mdr_env_t *env, const mdr_obs_spec_t *spec, const mdr_mlp_t *actor, uint64_t seed, uint64_t step,
                                    const int32_t *step_dev, int32_t greedy, int32_t max_workgroups, uint8_t *action, float *a_prob,
                                    float *probs, float *rows_out, void *stream);

/* ---- MADDPG with one network per agent (ddpg.py:200-213: every agent its own actor, critic and target of each; what every
 * checkpoint of saveDDPGDict holds).  At most MDR_MAX_AGENT_NETS nets per call: their weight pointers travel in the kernel argument
 * block (32 x 6 pointers = 1.5 KB), so no device table is owned by anybody and a captured call stays valid while the parameter
 * tensors stay where they are. */
#define MDR_MAX_AGENT_NETS 32

/* mdr_mlp_actor_sample with one actor per agent: row r of `obs` (nb_rows = envs x nb_nets rows, env-major: r = e nb_nets + k) goes
 * through net r % nb_nets.  `actors`: a HOST array of nb_nets descriptors in torch's own layout, all of one shape (num_state,
 * hidden1, hidden2; the limits of mdr_mlp_actor_sample), the weights read in place on every call.  Outputs, draw, `step_dev`, `greedy`
 * as there; the draw's counter is the GLOBAL row r, so a row's bits depend on the row, its net and (seed, step) only - with nb_nets
 * equal nets the call returns the bits of mdr_mlp_actor_sample on the same rows, and rows k, k + nb_nets, ... always equal
 * mdr_mlp_actor_sample(net k) on the whole batch.
 * A unit of work is (net k, tile of 32 envs): rows (32 t + j) nb_nets + k, F contiguous floats each, nb_nets ld_obs floats apart.  A
 * persistent workgroup holds net k's slabs of W1 and W2 in registers, walks a contiguous run of units and reloads the slabs only when
 * the run moves to the next net; the grid is min(units, compute units, max_workgroups if > 0) - with max_workgroups = 1 one workgroup
 * walks every net.  The outputs do not depend on the grid.  Stream-ordered, never synchronises, allocates nothing.
 * Returns 0; -1 (NULL `actors`, `obs` or `action`, a NULL weight pointer, a struct_size that is not this header's, nb_nets < 1,
 * nb_rows < 0, nb_rows not a multiple of nb_nets, max_workgroups < 0, ld_obs < F); -3 (HIP error); -4 (nb_nets >
 * MDR_MAX_AGENT_NETS, nets of differing shapes, a shape outside the limits).  On -1 and -4 nothing was launched and nothing written.
 * nb_rows == 0 returns 0 and launches nothing. */
int mdr_mlp_actors_sample(const mdr_mlp_t *actors, int32_t nb_nets, const float *obs, int64_t ld_obs, int64_t nb_rows, uint64_t seed,
                          uint64_t step, const int32_t *step_dev, int32_t greedy, int32_t max_workgroups, uint8_t *action, float *a_prob,
                          float *probs, void *stream);

/* mdr_maddpg_target with one target actor per agent (ddpg.py:282-284: agent k's next action comes from agent k's OWN target actor).
 * `tgt_actors`: a HOST array of nb_nets = nb_agents descriptors of one shape; `tgt_critic` is agent `agent`'s own target critic, one
 * net.  Everything else - rows, noise, outputs, the two launches - is mdr_maddpg_target's.  The pick launch tiles the picks per
 * agent: tile t holds agent k = t / ceil(nb_rows / 16) and the minibatch rows 16 (t mod ceil(nb_rows / 16)) + c, so that a tile's
 * MFMA A operand is one net; a row's arithmetic is a chain over k whatever its column, so next_action[:, k] has the bits
 * mdr_maddpg_target writes in column k when called with net k as its shared target actor, and with nb_nets equal nets every output
 * equals mdr_maddpg_target's bit for bit.
 * Returns as mdr_maddpg_target; -1 also for nb_nets != nb_agents; -4 also for nb_nets > MDR_MAX_AGENT_NETS and nets of differing
 * shapes.  On -1 and -4 nothing was launched and nothing written. */
int mdr_maddpg_target_agents(const mdr_mlp_t *tgt_actors, int32_t nb_nets, const mdr_mlp_t *tgt_critic, const float *next_state,
                             int64_t ld_state, const float *reward, const int64_t *index, int64_t nb_rows, int32_t nb_agents,
                             int32_t agent, const float *noise, float tau, float gamma, int32_t max_workgroups, float *y,
                             float *next_q, uint8_t *next_action, void *stream);

/* ---- The update of ALL agents in one pass, one actor, critic and target of each per agent.  With unshared nets the N steps of one
 * MADDPG.update() do not depend on each other: agent a's critic step reads critics[a], tgt_critics[a] and every tgt_actors[k] as the
 * PREVIOUS update left it, its actor step actors[a] and the stepped critics[a], and the targets are blended after the loop
 * (ddpg.py:300-339).  So the three calls below take the agent as a grid axis: tile t of a row pass is tile t mod TB of agent t / TB's
 * own minibatch (TB = ceil(nb_rows / 16)) and a weight-pass block's agent is the grid's y - N times the workgroups per launch, two
 * launches per call.  The nets of a kind are HOST arrays of nb_agents <= MDR_MAX_AGENT_NETS descriptors of one shape (the limits of
 * mdr_maddpg_target); their pointers travel in the kernel argument block (32 x 12 pointers = 3 KB), so nothing is allocated or owned
 * and a captured call stays valid while the tensors stay put.  The per-agent arrays are those mdr_maddpg_draws writes and their like:
 * `index` int64 [N][nb_rows] (required), the target's `noise` [N][nb_rows][N][2], the actor's [N][nb_rows][2], `y`, `next_q`, `q`
 * [N][nb_rows], `logits` [N][nb_rows][2], `next_action` uint8 [N][nb_rows][N], `grad` [N][mdr_maddpg_grad_floats], `loss` [N];
 * `workspace`: N times the single call's, 16-byte aligned (mdr_maddpg_workspace_bytes_all; agent a's part starts a whole share in).
 *
 * Slice a of every output holds, bit for bit, what mdr_maddpg_target_agents (agent = a, tgt_critics[a]), mdr_maddpg_critic_grad
 * (critics[a]) and mdr_maddpg_actor_grad (actors[a], critics[a], agent = a) write on index[a], noise[a], y[a], whatever
 * max_workgroups: a tile's work, the weight pass's sums in row order and the loss wave are the single calls' own code and none of
 * them knows the grid.  max_workgroups bounds the row pass's grid and, in the weight pass, the workgroups of ONE agent.
 * Stream-ordered, never synchronises.  Returns as mdr_maddpg_target_agents: 0; -1 (a NULL argument other than next_q / q / logits, a
 * struct_size that is not this header's, nb_agents < 1, shapes that do not fit each other (critic inputs != nb_agents (F + 2)),
 * nb_rows < 0, max_workgroups < 0, ld_state < nb_agents F, tau <= 0 or not finite, a workspace that is not 16-byte aligned); -3 (HIP
 * error); -4 (nb_agents > MDR_MAX_AGENT_NETS, nets of differing shapes, a shape outside the limits).  On -1 and -4 nothing was
 * launched and nothing written.  nb_rows == 0: as the single calls (the target launches nothing; the gradients are zeros, the
 * losses 0). */
int64_t mdr_maddpg_workspace_bytes_all(const mdr_mlp_t *actor, const mdr_mlp_t *critic, int32_t nb_agents, int64_t nb_rows,
                                       int32_t max_workgroups);
/* Launch one: every agent's picks for all N minibatches - mdr_maddpg_target_agents' pick launch over the N nb_rows concatenated rows
 * (a row's pick does not depend on its tile, so these tiles may straddle minibatches).  Launch two: y[a] = reward[:, a] + gamma
 * tgt_critics[a](next states, picks) on minibatch a. */
int mdr_maddpg_target_all(const mdr_mlp_t *tgt_actors, const mdr_mlp_t *tgt_critics, const float *next_state, int64_t ld_state,
                          const float *reward, const int64_t *index, int64_t nb_rows, int32_t nb_agents, const float *noise, float tau,
                          float gamma, int32_t max_workgroups, float *y, float *next_q, uint8_t *next_action, void *stream);
int mdr_maddpg_critic_grad_all(const mdr_mlp_t *critics, const float *state, int64_t ld_state, const int64_t *action,
                               const int64_t *index, int64_t nb_rows, int32_t nb_agents, const float *y, int32_t max_workgroups,
                               void *workspace, float *grad, float *loss, float *q, void *stream);
int mdr_maddpg_actor_grad_all(const mdr_mlp_t *actors, const mdr_mlp_t *critics, const float *state, int64_t ld_state,
                              const int64_t *action, const int64_t *index, int64_t nb_rows, int32_t nb_agents, const float *noise,
                              float tau, float pse, int32_t max_workgroups, void *workspace, float *grad, float *loss, float *q,
                              float *logits, void *stream);

/* ---- TarMAC-PPO's update step for the actor (TarmacPPO.update, agents/tarmac_ppo.py:168-186): loss and gradient of one minibatch.
 *
 * The actor's weights in torch's own layout - every layer w[out][in] contiguous and its bias, device memory, read as they are on
 * every call (the optimiser changes them between any two calls: no fragments, nothing to repack).  Activations as the reference:
 * ReLU inside obs2hidden and the head, tanh inside the three projections.  Limits (mdr_tarmac_actor_t's): F <= 64, H a multiple of
 * 4 <= 64, K a multiple of 4 <= 16, V a multiple of 4 <= 32, c = min(nb_comm, nb_houses - 1) <= 64, modes MDR_TARMAC_NEIGHBOURS
 * and MDR_TARMAC_NONE, num_hops == 1 (comm.msg_state2state is not evaluated).  with_comm == 0: obs2hidden -> hidden2action; K, V,
 * nb_comm, mode, defect_prob and the six projection layers are ignored (their pointers may be NULL). */
typedef struct mdr_tarmac_net {
  uint32_t struct_size;
  int32_t num_state;   /* F */
  int32_t hidden;      /* H */
  int32_t num_key;     /* K */
  int32_t num_value;   /* V */
  int32_t nb_comm;     /* number_agents_comm before the clamp to nb_houses - 1 */
  int32_t mode;        /* mdr_tarmac_mode */
  int32_t num_hops;    /* 1; anything else is MDR_ERR_UNSUPPORTED */
  int32_t with_comm;   /* 0 or 1 */
  float defect_prob;   /* comm_defect_prob, drawn as mdr_tarmac_comm documents */
  const float *encode_w0, *encode_b0, *encode_w2, *encode_b2; /* obs2hidden.0 [H][F], obs2hidden.2 [H][H] */
  const float *head_w0, *head_b0, *head_w2, *head_b2;         /* comm_hidden2action.0 [H][H + V] (columns: x, then comm), .2 [2][H];
                                                                  with_comm == 0: hidden2action.0 [H][H], .2 [2][H] */
  const float *key_w0, *key_b0, *key_w2, *key_b2;             /* comm.hidden2key.0 [H][H], .2 [K][H] */
  const float *value_w0, *value_b0, *value_w2, *value_b2;     /* comm.hidden2value.0 [H][H], .2 [V][H] */
  const float *query_w0, *query_b0, *query_w2, *query_b2;     /* comm.hidden2query.0 [H][H], .2 [K][H] */
} mdr_tarmac_net_t;

/* Floats of the flat gradient: the order of TarMACActor.parameters() (the reference's module order, network.py:201-222) restricted
 * to the tensors a one-hop evaluation reaches, each in torch's layout -
 *   obs2hidden.0.weight [H][F] | .0.bias [H] | .2.weight [H][H] | .2.bias [H]
 *   | comm_hidden2action.0.weight [H][H + V] | .0.bias [H] | .2.weight [2][H] | .2.bias [2]
 *   | comm.hidden2key.0.weight [H][H] | .0.bias [H] | .2.weight [K][H] | .2.bias [K]
 *   | comm.hidden2value.0.weight [H][H] | .0.bias [H] | .2.weight [V][H] | .2.bias [V]
 *   | comm.hidden2query.0.weight [H][H] | .0.bias [H] | .2.weight [K][H] | .2.bias [K]
 * comm.msg_state2state.* follows them in parameters() and is NOT part of it (one hop never evaluates it: autograd leaves its .grad
 * None).  with_comm == 0: obs2hidden's four, then hidden2action.0.weight [H][H] | .0.bias | .2.weight [2][H] | .2.bias [2].
 * Reads the shape fields, num_hops and with_comm only; host-only.  -1: a shape outside the limits, num_hops != 1, a struct_size
 * that is not this header's. */
int64_t mdr_tarmac_net_grad_floats(const mdr_tarmac_net_t *net);

/* Bytes of device scratch one gradient call over nb_rows env-steps of nb_houses agents (A = nb_rows * nb_houses) needs, in this
 * order, every part 16-byte aligned: one partial gradient (and loss) per tile slot - 2 slots per workgroup of the grid
 * min(ceil(A / 32), max_workgroups), with max_workgroups == 0 enough for the library's own grid on any device - | the head's input
 * [x | comm] [A][H + V] | d[x | comm] [A][H + V] | packed q | k | v [A][2 K + V] | packed dq | dk | dv [A][2 K + V] | the attention
 * backward's statistics, mdr_tarmac_comm_backward_workspace_bytes(A, K, V), reserved inside: there is ONE workspace pointer.
 * with_comm == 0: the partials | x [A][H] | dx [A][H].  Host-only.  -1 as above, or nb_rows < 0, nb_houses <= 0, max_workgroups < 0,
 * A >= 2^31 - 16. */
int64_t mdr_tarmac_ppo_workspace_bytes(const mdr_tarmac_net_t *net, int64_t nb_rows, int32_t nb_houses, int32_t max_workgroups);

/* The clipped surrogate of agents/tarmac_ppo.py:168-182 and its gradient.  Minibatch row i < nb_rows is the stored env-step
 * j = index ? index[i] : i (`index` device int64, may be NULL); its N = nb_houses agents are rows j * N + n of `state` (F floats each,
 * ld_state >= F), of `action` (int64, nonzero = action 1) and of `old_prob` (the stored probability of the taken action) -
 * whole-buffer arrays read in place through `index`; `advantage` float [nb_rows][N] in minibatch order.
 * p = softmax(actor(state_j)) - the row's N agents attend to each other -, ratio_in = p_n[action] / old_prob,
 *   loss = -(1 / (nb_rows N)) sum_in min(ratio_in A_in, clamp(ratio_in, 1 - clip_param, 1 + clip_param) A_in)
 * and `grad` (mdr_tarmac_net_grad_floats floats) = d loss / d parameters as torch's autograd takes it: d loss / d ratio =
 * -A / (nb_rows N) where 1 - clip <= ratio <= 1 + clip (bounds included) or ratio A < clamp(ratio) A, else 0; relu'(z) = 1 iff
 * z > 0.  old_prob = 0 gives inf / NaN as in the reference.  `loss`: one float on the device.  `ratio` (may be NULL): float
 * [nb_rows][N].  Dead senders (defect_prob > 0): minibatch row i stands for the env in the Philox key of mdr_tarmac_comm, the forward
 * and the backward attention of one call use the same (seed, step, hop 0) - the evaluation TarMACActor.forward(state[index], seed =
 * seed, step = step, differentiable = True) makes.
 * Exact fp32 on v_mfma_f32_16x16x4_f32, no library GEMM.  The chain (csrc/mdr_tarmac_ppo_grad.hip): obs2hidden forward, projections
 * forward, mdr_tarmac_comm, the head's forward + loss + backward, mdr_tarmac_comm_backward, projections backward (tanh recomputed
 * from x), obs2hidden backward (relu recomputed from the observation rows), one reduction; without communication obs2hidden
 * forward, head, obs2hidden backward, reduction.  Every compute kernel runs on the same persistent grid of min(ceil(A / 32),
 * max_workgroups) workgroups (0: the library's choice, min(.., compute units, 512)), each leaving two partial gradients in
 * `workspace`; the reduction adds them in slot order and divides by nb_rows N: no floating-point atomics, the same inputs and the
 * same max_workgroups give the same bits on every call.  Every float of `grad`, `loss` and `ratio` is written by every successful
 * call; nb_rows == 0 writes zeros to `grad` and `loss`.  Stream-ordered, never synchronises, allocates nothing; `workspace`:
 * 16-byte aligned device memory of mdr_tarmac_ppo_workspace_bytes, owned by the caller, its contents free before and after.
 * Returns 0; -1 (a NULL required pointer, ld_state < F, nb_rows < 0, nb_houses <= 0, nb_comm < 0, max_workgroups < 0, clip_param
 * outside [0, 1), defect_prob outside [0, 1], a struct_size that is not this header's, a missing or misaligned workspace); -3 (HIP
 * error); -4 (a shape outside the limits, another mode, num_hops != 1, c > 64, A >= 2^31 - 16).  On -1 and -4 nothing was launched
 * and nothing written. */
int mdr_tarmac_ppo_actor_grad(const mdr_tarmac_net_t *net, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                              int32_t nb_houses, const int64_t *action, const float *old_prob, const float *advantage, float clip_param,
                              uint64_t seed, uint64_t step, int32_t max_workgroups, void *workspace, float *grad, float *loss,
                              float *ratio, void *stream);

/* The same call with the key of the dead-sender draw from device memory (`key_dev` int32 [2] = seed low word, seed high word, as
 * mdr_tarmac_comm_keyed reads it) and `step_dev` (device int32, may be NULL) added to the low word of `step` when the kernels run;
 * both are handed to the two attention calls of the chain, no other kernel draws.  key_dev = the words of `seed` and
 * step + *step_dev = the by-value `step` (below 2^32: the sum wraps in the low word) give mdr_tarmac_ppo_actor_grad's bits.  A NULL
 * `key_dev` is -1 with nothing launched and nothing written. */
int mdr_tarmac_ppo_actor_grad_keyed(const mdr_tarmac_net_t *net, const float *state, int64_t ld_state, const int64_t *index,
                                    int64_t nb_rows, int32_t nb_houses, const int64_t *action, const float *old_prob,
                                    const float *advantage, float clip_param, const int32_t *key_dev, uint64_t step,
                                    const int32_t *step_dev, int32_t max_workgroups, void *workspace, float *grad, float *loss,
                                    float *ratio, void *stream);

/* ---- TarMAC-PPO's update step for the centralised critic (TarmacPPO.update, agents/tarmac_ppo.py:159-166, 196-204): value,
 * advantage, value loss and gradient of one minibatch.
 *
 * The critic is TarMAC_Critic (agents/network.py:241-259), Linear(N F, H1) - ReLU - Linear(H1, H2) - ReLU - Linear(H2, N), as
 * mdr_mlp_t in torch's own layout with num_state = J = N F and num_out = N (the number of agents: one value each), read as it is
 * on every call.  Limits: J <= 4096 (50 houses of 51 features: 2550), every hidden layer <= 256 units of any size (no multiple of
 * 16 needed), 1 <= N <= 64.  The weights are streamed from L2 in the manner of the MADDPG calls (csrc/mdr_tarmac_critic_grad.hip;
 * the device helpers both share are csrc/mdr_stream_mlp.h), whose limits and bits are unchanged.
 *
 * Rows.  Minibatch row i < nb_rows is stored env-step j = index ? index[i] : i (`index` device int64, may be NULL); its input is the
 * J contiguous floats at `state` + j * ld_state (ld_state >= J) - N agents of F floats each in agent order, the buffer
 * mdr_tarmac_ppo_actor_grad reads with nb_houses = N and ld_state = F: no joint tensor is built.  `target`: the whole return buffer,
 * float [env-steps][N], gathered through the same `index`.
 *   V_i = critic(x_i);  delta_ik = target[j][k] - V_ik (rounded once);  advantage_ik = delta_ik;
 *   loss = (sum_ik delta_ik^2) / (float)(nb_rows N)      (torch.pow(delta, 2).mean(0).mean(0))
 *   d loss / d V_ik = (-2 delta_ik) inv,  inv = the fp32 value of 1 / (nb_rows N) formed on the host in double: ONE scale where
 *   autograd's mean(0).mean(0) divides by nb_rows and then by N;  relu'(z) = 1 iff z > 0.
 * Exact fp32 on v_mfma_f32_16x16x4_f32, no floating-point atomics, no signalling between workgroups; the same inputs and the same
 * max_workgroups give the same bits on every call, and every element of every given output is written by every successful call.
 * Row pass: a workgroup of 1024 threads takes floor(16 / nb) tiles of 16 rows at once, nb = the most 16-unit blocks of H1, H2 and N
 * (four tiles at the reference's 64 hidden units), all against the same streamed weights; a persistent grid of min(ceil(tiles /
 * tiles per workgroup), max_workgroups) workgroups (0: the library's choice, at most min(compute units, 512)).  A row's bits depend
 * neither on its place in a workgroup nor on the grid.  Stream-ordered, never synchronise, allocate nothing.
 *
 * Floats of the flat gradient, dW1 | db1 | dW2 | db2 | dW3 | db3 in torch's parameter order and layout (host-only).  -1: a NULL net,
 * num_out < 1, num_state % num_out != 0, a size <= 0, a shape outside the limits, a struct_size that is not this header's. */
int64_t mdr_tarmac_critic_grad_floats(const mdr_mlp_t *critic);
/* Bytes of device scratch mdr_tarmac_critic_grad needs over nb_rows rows, with Bp = nb_rows rounded up to 16: h1, dz1 [Bp][pad16(H1)]
 * | h2, dz2 [Bp][pad16(H2)] | dV [Bp][pad16(N)] | the rows' loss terms [Bp] (host-only, independent of max_workgroups).  -1 as
 * above, or nb_rows < 0, max_workgroups < 0. */
int64_t mdr_tarmac_critic_workspace_bytes(const mdr_mlp_t *critic, int64_t nb_rows, int32_t max_workgroups);

/* The forward alone (TarmacPPO.get_value, agents/tarmac_ppo.py:97-104, and the bootstrap): `value` float [nb_rows][N] = V, bit for
 * bit the `value` of mdr_tarmac_critic_grad on the same rows.  One launch, no workspace; nb_rows == 0 launches nothing.
 * Returns 0; -1 (a NULL required pointer, num_out < 1, num_state % num_out != 0, a size <= 0, ld_state < J, nb_rows < 0,
 * max_workgroups < 0, a struct_size that is not this header's); -3 (HIP error); -4 (a shape outside the limits).  On -1 and -4
 * nothing was launched and nothing written. */
int mdr_tarmac_critic_value(const mdr_mlp_t *critic, const float *state, int64_t ld_state, const int64_t *index, int64_t nb_rows,
                            int32_t max_workgroups, float *value, void *stream);

/* The critic's step: `loss` (one float on the device) and `grad` (mdr_tarmac_critic_grad_floats floats) = d loss / d parameters as
 * autograd takes it; `value` and `advantage` (each may be NULL) float [nb_rows][N] in minibatch order - `advantage` is what
 * mdr_tarmac_ppo_actor_grad takes.  A NaN in `target` reaches `advantage`, `loss` and `grad`, never `value`.  `workspace`: 16-byte
 * aligned device memory of mdr_tarmac_critic_workspace_bytes, owned by the caller, its contents free before and after the call.
 * Two launches: the row pass, then a weight pass of one wave per 16 x 16 block of a weight gradient, summing over the minibatch rows
 * in row order (at most max_workgroups workgroups of four waves; 0: one wave per block), one more wave adding the rows' loss terms
 * in a fixed order.  nb_rows == 0 writes zeros to `grad` and `loss` (the weight pass alone) and leaves `value` and `advantage`.
 * Returns 0; -1 (as mdr_tarmac_critic_value, or a missing or misaligned workspace); -3; -4.  On -1 and -4 nothing was launched and
 * nothing written. */
int mdr_tarmac_critic_grad(const mdr_mlp_t *critic, const float *state, int64_t ld_state, const float *target, const int64_t *index,
                           int64_t nb_rows, int32_t max_workgroups, void *workspace, float *grad, float *loss, float *value,
                           float *advantage, void *stream);

/* ---- TarMAC A2C (the reference's train_tarmac.py): MultiAgentPolicy (agents/tarmac/model.py:132-266) as A2C_ACKTR builds it
 * (agents/tarmac/a2c_acktr.py:35-36: no GRU, one hop) - the act step and the update step of update_multi_agent (a2c_acktr.py:59-107).
 *
 * The network in torch's own layout (w[out][in] contiguous, device memory, read as it is on every call), F = num_obs, C = num_comm,
 * S = state_size, K = num_key:  common_w0 [S][F + C], common_b0 [S], common_w2 [S][S], common_b2 [S] (base.common.0 / .2);
 * critic_w0 [S][S], critic_b0 [S], critic_w3 [1][S], critic_b3 [1] (base.critic.0 / .3); query_w, key_w [K][S], query_b, key_b [K],
 * value_w [C][S], value_b [C] (base.comm.state2query / state2key / state2value); dist_w [2][S] (dist.linear, no bias).
 * Limits: 1 <= F <= 128, C a multiple of 4 <= 32, S a multiple of 4 <= 128, K a multiple of 4 <= 16, 1 <= N <= 64 agents per env,
 * at most 2^24 env-steps per call, one hop (base.comm.msg2nextstate is not reached and has no place here).
 *
 * One env-step b of N agents, row r = b N + n, LeakyReLU slope 0.01:
 *   in = [obs | comm_in];  h1 = leaky(W1 in + b1);  x = W2 h1 + b2;  logits = Wd x;
 *   xbar_b = (sum_n x_bn, agent order) / N;  V_b = Wc2 leaky(Wc1 xbar_b + bc1) + bc2     (the critic's first layer is linear before
 *   MeanAll: the mean is taken first - ONE value per env-step);
 *   q = Wq x + bq, k = Wk x + bk, v = Wv x + bv;  attn_ij = softmax_j(q_i k_j / sqrt(C)) over ALL agents j of the env, j = i included
 *   (the scale is sqrt(C), model.py:115-116);  comm_out_i = sum_j attn_ij v_j.
 * Exact fp32 (the MLPs on v_mfma_f32_16x16x4_f32, the weights streamed from L2; csrc/mdr_tarmac_a2c.hip), no library GEMM, no
 * floating-point atomics, no partial sums whose order depends on the grid: the bits of every output are independent of
 * max_workgroups (0: the library's choice) and of where `index` points.  Stream-ordered, never synchronise, allocate nothing.
 * Returns of the three compute calls: 0; -1 (a NULL required pointer, a misaligned workspace or x, ld_obs < F, ld_comm < C (ld_out <
 * C), nb_steps < 0, nb_agents < 1, max_workgroups < 0, a size < 1, a struct_size that is not this header's); -3 (HIP error); -4 (a
 * shape outside the limits).  On -1 and -4 nothing was launched and nothing written. */
typedef struct mdr_tarmac_a2c_net {
  uint32_t struct_size;
  int32_t num_obs, num_comm, state_size, num_key;
  const float *common_w0, *common_b0, *common_w2, *common_b2;
  const float *critic_w0, *critic_b0, *critic_w3, *critic_b3;
  const float *query_w, *query_b, *key_w, *key_b, *value_w, *value_b;
  const float *dist_w;
} mdr_tarmac_a2c_net_t;

/* Floats of the flat gradient: the nine tensors an update reaches, in parameters() order - common_w0 | common_b0 | common_w2 |
 * common_b2 | critic_w0 | critic_b0 | critic_w3 | critic_b3 | dist_w (evaluate_actions discards the new communication: query, key
 * and value get no gradient).  Host-only.  -1: a NULL net, a size < 1, a shape outside the limits, another struct_size. */
int64_t mdr_tarmac_a2c_grad_floats(const mdr_tarmac_a2c_net_t *net);
/* Bytes of device scratch over nb_steps env-steps of nb_agents agents, with Rp = nb_steps nb_agents and Bp = nb_steps rounded up to
 * 16, Sp = S rounded up to 16 (floats): h1 | x | dx | dz1 [Rp][Sp], logits | dlogits [Rp][2], xbar | a | da | dxbar / N [Bp][Sp], dV
 * [Bp], the env-steps' loss terms [Bp][4].  Rows past the batch hold exact zeros after mdr_tarmac_a2c_grad.  Host-only, independent of
 * max_workgroups.  -1 as above, or nb_steps < 0, nb_agents outside 1..64, max_workgroups < 0. */
int64_t mdr_tarmac_a2c_workspace_bytes(const mdr_tarmac_a2c_net_t *net, int64_t nb_steps, int32_t nb_agents, int32_t max_workgroups);

/* The forward of MultiAgentBase.forward + dist (model.py:169-183, 244-266) without the communication: minibatch env-step i < nb_steps
 * is stored env-step j = index ? index[i] : i (`index` device int64, may be NULL); its agent n is row j N + n of `obs` (F floats, row
 * stride ld_obs >= F) and of `comm_in` (C floats, row stride ld_comm >= C) - two buffers, never concatenated in memory.  `logits`
 * float [nb_steps N][2], `value` float [nb_steps], `x` (may be NULL; 16-byte aligned) float [nb_steps N][S].  Bit for bit the logits
 * and the value mdr_tarmac_a2c_grad forms on the same rows.  `workspace` (mdr_tarmac_a2c_workspace_bytes, 16-byte aligned) is
 * needed only where `x` is NULL.  Two launches (the row pass, the env-step pass); nb_steps == 0 launches nothing. */
int mdr_tarmac_a2c_forward(const mdr_tarmac_a2c_net_t *net, const float *obs, int64_t ld_obs, const float *comm_in, int64_t ld_comm,
                           const int64_t *index, int64_t nb_steps, int32_t nb_agents, int32_t max_workgroups, void *workspace,
                           float *logits, float *value, float *x, void *stream);

/* CommAttention.forward (model.py:88-129) for one hop: `x` float [nb_envs N][S] (contiguous) -> `comm_out` float [nb_envs N][C] (row
 * stride ld_out >= C: a slab of the next step's comm_in) and `attn` (may be NULL) float [nb_envs][N][N].  One workgroup per env
 * (persistent over the envs), x, q, k and v of the env in LDS; the row softmax subtracts the row's maximum and adds the exponentials
 * in ascending j; every contraction in ascending order on one accumulator.  One launch; nb_envs == 0 launches nothing. */
int mdr_tarmac_a2c_comm(const mdr_tarmac_a2c_net_t *net, const float *x, int64_t nb_envs, int32_t nb_agents, int32_t max_workgroups,
                        float *comm_out, int64_t ld_out, float *attn, void *stream);

/* The update's loss and gradient over nb_steps env-steps (count = nb_steps N): `action` (int64, nonzero = action 1) and `ret`
 * (float) are the whole buffers [env-steps][N], gathered through `index` like obs and comm_in.
 *   delta_bn = ret_bn - V_b;  d = l_taken - l_other, t = exp(-|d|), p_taken / p_other = 1 / (1 + t) and t / (1 + t) by the sign of d,
 *   -log p_taken = max(-d, 0) + log1p(t), H = -(p_taken log p_taken + p_other log p_other);
 *   losses[0] = value_loss = sum delta^2 / count, losses[1] = action_loss = -sum delta log p_taken / count (delta detached),
 *   losses[2] = entropy = sum H / count;  `grad` (mdr_tarmac_a2c_grad_floats floats) = d (value_coef value_loss + action_loss -
 *   entropy_coef entropy) / d parameters as autograd takes it; leaky'(z) = 1 for z > 0, 0.01 otherwise.
 * `value` float [nb_steps], `advantage` float [nb_steps][N] = delta (each may be NULL).  A NaN in `ret` reaches the losses, the
 * gradient and `advantage`, never `value`.  Four launches: row pass, env-step pass, row pass backward, and a weight pass of one wave
 * per 16 x 16 block of a weight gradient summing over the rows in row order (at most max_workgroups workgroups of four waves; 0: one
 * wave per block), one more wave adding the env-steps' loss terms in a fixed order.  Every element of every given output is written
 * by every successful call; nb_steps == 0 launches no kernel and writes zeros to `grad` and `losses`. */
int mdr_tarmac_a2c_grad(const mdr_tarmac_a2c_net_t *net, const float *obs, int64_t ld_obs, const float *comm_in, int64_t ld_comm,
                        const int64_t *action, const float *ret, const int64_t *index, int64_t nb_steps, int32_t nb_agents,
                        float value_coef, float entropy_coef, int32_t max_workgroups, void *workspace, float *grad, float *losses,
                        float *value, float *advantage, void *stream);

/* ---- The optimiser tail of every update: clamp, norm clip, Adam and the target blend in one launch (csrc/mdr_optim.hip).
 *
 * A network's tensors as a table of segments: `param` (device float [count], updated in place), `grad` (device float [count], read
 * only; NULL: the segment is skipped entirely, as torch.optim.Adam skips p.grad is None - its parameter, moments and target stay
 * untouched and it is no part of the norm), `target` (device float [count], NULL where no blend is asked for).  Any float alignment:
 * slices of one flat gradient buffer and separately allocated tensors are both fine. */
#define MDR_ADAM_MAX_SEGMENTS 32
typedef struct mdr_adam_segment {
  float *param;
  const float *grad;
  float *target;
  int64_t count;
} mdr_adam_segment_t;

typedef struct mdr_adam_segments {
  uint32_t struct_size;
  int32_t nb_segments; /* <= MDR_ADAM_MAX_SEGMENTS */
  mdr_adam_segment_t seg[MDR_ADAM_MAX_SEGMENTS];
} mdr_adam_segments_t;

/* Bytes of device scratch a call over segments of total_floats elements in all may need (the chunk sums of the two-launch form),
 * a multiple of 16.  Host-only.  -1: total_floats < 0. */
int64_t mdr_adam_workspace_bytes(int64_t total_floats);

/* One step of torch.optim.Adam (betas, eps as given; no weight decay, no amsgrad) on every live segment, from the gradient on the
 * device, with nothing read back.  `exp_avg`, `exp_avg_sq`: device float [sum of all counts], the segments' moments one after the
 * other in segment order (dead segments keep their place).  Per element, in fp32:
 *   g = grad clamped to [-grad_clamp, grad_clamp] by comparisons (v < -c ? -c : v > c ? c : v: a NaN stays a NaN; INFINITY: no clamp)
 *   max_grad_norm > 0 and finite: total_norm = sqrt(sum g^2) over the live segments, coef = max_grad_norm / (total_norm + 1e-6),
 *     at most 1 (c > 1 ? 1 : c: a NaN total_norm gives a NaN coef), g = coef g - nn.utils.clip_grad_norm_ with
 *     error_if_nonfinite=False; <= 0 or INFINITY: no clip
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   param = param - (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *   tau > 0: target = (1 - tau) target + tau param, with the new param (agents/dqn.py:77-82); <= 0: no blend
 * The constants (1 - beta, the two bias corrections, 1 - tau) are formed on the host in double and passed as floats.  `grad` is
 * NEVER written: after the call it still holds the unclipped, unclamped gradient - the one visible difference from
 * clip_grad_norm_, which scales .grad in place.  `total_norm_out` (may be NULL): one device float, total_norm (of the clamped
 * gradient; written with or without a clip).
 * The norm is deterministic, no floating-point atomics: chunks of 1024 consecutive elements of one live segment (the last of a
 * segment ragged), each summed by one wave in a fixed order, the chunk sums added in chunk order - the same bits whatever the grid
 * and whichever form ran.  Forms: the sum of all counts <= max_fused_floats (0: the library's measured default) - ONE launch, every
 * workgroup recomputes the norm and steps its own chunks; larger - TWO launches, chunk sums into `workspace`
 * (mdr_adam_workspace_bytes, 16-byte aligned, required by this form only), then sum and step.  Neither clip nor total_norm_out: no
 * norm pass, one launch at any size.  Stream-ordered, never synchronises, allocates nothing.
 * Returns 0; -1 (a NULL segments / exp_avg / exp_avg_sq / param pointer, a struct_size that is not this header's, nb_segments < 0,
 * a negative count, step < 1, tau > 0 with a live segment without target, tau > 1, betas outside [0, 1), eps < 0, grad_clamp NaN
 * or <= 0, max_fused_floats < 0, a missing or misaligned workspace for the two-launch form); -3 (HIP error); -4 (more than
 * MDR_ADAM_MAX_SEGMENTS segments, 2^30 chunks or more).  On -1 and -4 nothing was launched and nothing written. */
int mdr_adam_step(const mdr_adam_segments_t *segments, float *exp_avg, float *exp_avg_sq, double lr, double beta1, double beta2,
                  double eps, int64_t step, double max_grad_norm, double grad_clamp, double tau, void *workspace,
                  float *total_norm_out, int32_t max_fused_floats, void *stream);

/* The two bias corrections of mdr_adam_step as it forms them on the host, for the steps first_step .. first_step + count - 1:
 *   out[2 k]     = (float)(lr / (1 - pow(beta1, step)))      step_size
 *   out[2 k + 1] = (float)sqrt(1 - pow(beta2, step))         bc2_sqrt       step = first_step + k, in double, one cast to float
 * - the very expressions, so the entries are that function's bits.  Host-only, no device call.  Returns 0; -1 (out NULL, first_step
 * < 1, count < 0, lr NaN, betas outside [0, 1)). */
int mdr_adam_corrections(double lr, double beta1, double beta2, int64_t first_step, int64_t count, float *out_host_floats);

/* mdr_adam_step with the bias corrections read from device memory, so that a launch captured into a graph takes another step's
 * corrections at every replay: `corrections` (device float pairs {step_size, bc2_sqrt}, mdr_adam_corrections' uploaded by the
 * caller), pair number slot + (base_dev ? *base_dev : 0) (`base_dev`: one device int32, may be NULL; the caller keeps the sum inside
 * the table - the kernel cannot know its length).  `lr` is not read beyond the NaN check: the table carries it.  Everything else -
 * the arithmetic, the forms, the workspace, the return codes - as mdr_adam_step, and the same bits as its call with the step whose
 * pair is read; additionally -1 for corrections NULL or slot < 0. */
int mdr_adam_step_table(const mdr_adam_segments_t *segments, float *exp_avg, float *exp_avg_sq, double lr, double beta1, double beta2,
                        double eps, const float *corrections, int32_t slot, const int32_t *base_dev, double max_grad_norm,
                        double grad_clamp, double tau, void *workspace, float *total_norm_out, int32_t max_fused_floats, void *stream);

/* mdr_adam_step for N nets at once - the N critics, then the N actors of MADDPG's per-agent networks: clip and Adam of all of them in
 * at most two launches, every net with its own total norm, its own clip and its own target blend.  One net's segment records are
 * 1.5 KB, so those of N nets live in a device TABLE the caller owns: mdr_adam_nets_table_bytes(nb_nets) bytes, 16-byte aligned.
 * mdr_adam_nets_bind writes record `net` (0 <= net < the nb_nets the table was sized for - the library cannot check that) from
 * `segments` (mdr_adam_step's own table, a NULL grad a dead segment, targets NULL or all set) and the net's two moment buffers: one
 * small launch whose values are its kernel arguments, stream-ordered; call it once per net and again only when an address changes.
 * mdr_adam_step_nets steps the nets 0 .. nb_nets - 1 of the table with one set of hyper-parameters and ONE step count (nets at
 * different counts take mdr_adam_step each): launch one writes the chunk sums of every net to `workspace` (nb_nets x
 * mdr_adam_workspace_bytes(max_net_floats) bytes, 16-byte aligned; skipped with neither clip nor total_norm_out), launch two adds
 * each net's own chunk sums in chunk order and steps it.  `max_net_floats`: an upper bound of the floats of every bound net (it sizes
 * the grid and the workspace's shares; a net bound with more chunks than a share holds is left untouched).  tau > 0 blends the nets
 * bound with targets.  `total_norm_out`: float [nb_nets] or NULL.  The chunks, the sums and the element's expressions are
 * mdr_adam_step's, so every net's parameters, moments, targets and norm are, bit for bit, those of mdr_adam_step on that net alone.
 * Return codes as mdr_adam_step; nb_nets == 0 returns 0. */
int64_t mdr_adam_nets_table_bytes(int32_t nb_nets);
int mdr_adam_nets_bind(void *table, int32_t net, const mdr_adam_segments_t *segments, float *exp_avg, float *exp_avg_sq, void *stream);
int mdr_adam_step_nets(const void *table, int32_t nb_nets, int64_t max_net_floats, double lr, double beta1, double beta2, double eps,
                       int64_t step, double max_grad_norm, double grad_clamp, double tau, void *workspace, float *total_norm_out,
                       void *stream);

/* ---- Minibatch indices drawn on the device (csrc/mdr_minibatch.hip), so that a whole update can be captured into a graph.
 *
 * A permutation of 0 .. n - 1 into `out` (device int64 [n]), one thread per element, no sort: a balanced Feistel network with
 * cycle walking.  b = max(1, ceil(log2 n)), h = ceil(b / 2); the domain is the 2h-bit integers (fewer than 4 n of them for n > 1).
 * Element i: x = i; x = feistel(x) until x < n; out[i] = x.  feistel: L = x >> h, R = x & (2^h - 1); four rounds r = 0..3 of
 * (L, R) = (R, L ^ (F(r, R) & (2^h - 1))); the result is (L << h) | R.  F(r, R) = word .x of Philox4x32-10 on the counter
 * (R, r, epoch lo + *cursor_dev, MDR_TAG_MINIBATCH ^ epoch hi) under the key (seed lo, seed hi).  A balanced Feistel network is a
 * bijection whatever F is, and cycle walking keeps it one on [0, n).  `cursor_dev` (may be NULL): one device int32 added to the low
 * word of `epoch` (mod 2^32, no carry), read when the kernel runs - a captured launch draws a new permutation at every replay.
 * The _keyed form reads the key from the device as well: key_dev[0] = seed lo, key_dev[1] = seed hi (device int32 [2]).
 * n == 0 launches nothing.  Stream-ordered, never synchronises, allocates nothing.
 * Returns 0; -1 (n < 0, out NULL with n > 0, key_dev NULL); -3 (HIP error); -4 (n >= 2^62). */
#define MDR_TAG_MINIBATCH 0x4D425031u /* "MBP1" */
#define MDR_TAG_REPLAY 0x4D425331u    /* "MBS1" */
int mdr_minibatch_permutation(int64_t n, uint64_t seed, uint64_t epoch, const int32_t *cursor_dev, int64_t *out, void *stream);
int mdr_minibatch_permutation_keyed(int64_t n, const int32_t *key_dev, uint64_t epoch, const int32_t *cursor_dev, int64_t *out,
                                    void *stream);

/* nb positions drawn uniformly with replacement from [0, len) into `out` (device int64 [nb]) - random.choices, agents/buffer.py:26-27:
 * out[i] = (word * len) >> 32 with word = .x of Philox4x32-10 on the counter (i lo, i hi, step lo + *cursor_dev, MDR_TAG_REPLAY ^ step hi)
 * under the key (seed lo, seed hi).  `len_dev` (may be NULL: `len` is taken): one device int64 read when the kernel runs, so that a
 * captured launch follows a growing buffer; either way 1 <= len <= 2^32 - 1 (a device value outside that range is clamped into it:
 * the kernel cannot refuse).  The multiply-high maps 2^32 words onto len values, so some values are hit once more often than others:
 * the bias of any value's probability is at most len / 2^32 relative (1.2e-4 at len = 524288).  _keyed: the key from the device, as above.
 * nb == 0 launches nothing.  Returns 0; -1 (nb < 0, out NULL with nb > 0, len_dev NULL with len outside [1, 2^32 - 1], key_dev
 * NULL); -3 (HIP error). */
int mdr_minibatch_sample(int64_t nb, const int64_t *len_dev, int64_t len, uint64_t seed, uint64_t step, const int32_t *cursor_dev,
                         int64_t *out, void *stream);
int mdr_minibatch_sample_keyed(int64_t nb, const int64_t *len_dev, int64_t len, const int32_t *key_dev, uint64_t step,
                               const int32_t *cursor_dev, int64_t *out, void *stream);

/* Everything one MADDPG update draws (MADDPGLearner.draws: a fresh minibatch per agent, ddpg.py:268, 307, and the gumbel noise of
 * every F.gumbel_softmax of the update), in ONE launch.  With c2 = step lo + *cursor_dev (mod 2^32, no carry), c3 = TAG ^ step hi and
 * the key (k0, k1) = (seed lo, seed hi):
 * `index` int64 [nb_agents][batch]: index[a][i] = element i of the permutation of mdr_minibatch_permutation over `len` elements - the
 *   same Feistel network and cycle walk - with the round function word .x of Philox4x32-10 on the counter (R, (a << 8) | r, c2,
 *   MDR_TAG_MADDPG_INDEX ^ step hi): `batch` DISTINCT positions below len per agent (np.random.choice(len, batch, replace=False)),
 *   no sort, no scratch.  `len_dev` (may be NULL: `len` is taken): one device int64 read when the kernel runs, h = ceil(max(1,
 *   ceil(log2 len)) / 2) then computed on the device; a device len < 1 is read as 1 (>= 2^62: as 2^62 - 1), and where it is below
 *   `batch` the walk of element i starts at i mod len - such rows repeat positions, no position >= len is ever stored and no
 *   walk is endless (a walk that starts below len returns to its start).
 * `noise_t` float [nb_agents][batch][nb_agents][2], `noise_a` float [nb_agents][batch][2]: Gumbel(0, 1) noise, contiguous, as
 *   mdr_maddpg_target[_agents] and mdr_maddpg_actor_grad read it per agent slice.  For q = (a batch + b) (nb_agents + 1) + k the words
 *   .x, .y of Philox4x32-10 on the counter (q lo, q hi, c2, MDR_TAG_MADDPG_NOISE ^ step hi) give components 0 and 1 of
 *   noise_t[a][b][k] (k < nb_agents) or noise_a[a][b] (k = nb_agents); the value is (float)(-log(-log(u))) with u = (word + 0.5) / 2^32,
 *   evaluated in double (in fp32 u rounds to 1 for the top words and the noise would be infinite): finite, in about [-3.2, 22.9].
 * nb_agents <= MDR_MADDPG_DRAWS_MAX_AGENTS = 1280 / 3: what mdr_maddpg_target's joint input of nb_agents (F + 2) <= 1280 columns
 * admits at F = 1.  _keyed: the key from the device (int32 [2]), as above.  batch == 0 launches nothing.  Stream-ordered, never
 * synchronises, allocates nothing.
 * Returns 0; -1 (nb_agents < 1, batch < 0, a NULL output with batch > 0, len_dev NULL with len < 1 or batch > len, key_dev NULL);
 * -3 (HIP error); -4 (nb_agents > MDR_MADDPG_DRAWS_MAX_AGENTS, len >= 2^62, more than 2^31 - 1 workgroups). */
#define MDR_TAG_MADDPG_INDEX 0x4D444931u /* "MDI1" */
#define MDR_TAG_MADDPG_NOISE 0x4D444E31u /* "MDN1" */
#define MDR_MADDPG_DRAWS_MAX_AGENTS 426
int mdr_maddpg_draws(int32_t nb_agents, int64_t batch, const int64_t *len_dev, int64_t len, uint64_t seed, uint64_t step,
                     const int32_t *cursor_dev, int64_t *index, float *noise_t, float *noise_a, void *stream);
int mdr_maddpg_draws_keyed(int32_t nb_agents, int64_t batch, const int64_t *len_dev, int64_t len, const int32_t *key_dev, uint64_t step,
                           const int32_t *cursor_dev, int64_t *index, float *noise_t, float *noise_a, void *stream);

/* The device block such captured launches read their cursors from, written stream-ordered by one-thread kernels whose values are
 * kernel arguments (copied at launch: no staging buffer that could be overwritten too early).  _set: dst[k] = v_k for k < count
 * (1 <= count <= 4); _add: dst[index] += delta.  Returns 0; -1 (dst NULL, count outside 1..4, index < 0); -3 (HIP error). */
int mdr_update_cursor_set(int32_t *dst, int32_t count, int32_t v0, int32_t v1, int32_t v2, int32_t v3, void *stream);
int mdr_update_cursor_add(int32_t *dst, int32_t index, int32_t delta, void *stream);

#ifdef __cplusplus
}
#endif
#endif
