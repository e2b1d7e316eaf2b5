/* magpo.h -- C ABI of libmagpo_hip.so: the MI355X (gfx950) kernels behind the MAGPO Anakin learner.
 *
 * The reference (liyheng/MAGPO) has no FFI: its hot path is one jitted XLA program behind the Python
 * callable `learn: LearnerFn[GPOLearnerState]` (mava/systems/gpo/anakin/rec_magpo.py:91-530, :635-636).
 * This header is the boundary a maintainer binds instead (ctypes stub: INTEGRATION.md); every entry
 * point names the reference computation it replaces.
 *
 * Conventions
 *   - plain C types only; all pointers are DEVICE pointers unless the name ends in _host;
 *   - fp32 row-major; `ld*` / `*_stride` are element strides; `hipStream_t` is passed as void*;
 *   - stream-ordered and asynchronous; no allocation, no host synchronisation; no setters, no environment variables and no
 *     mutable library state that changes results or buffer sizes: every tuning knob (retention chunk size, GRU MFMA mode and block
 *     rows, A/B kernel variants, acting envs per wave) is a per-call argument.  The only process-level state is the thread-local
 *     error string and memoised device queries (occupancy caps, raised dynamic-LDS limits: idempotent);
 *   - return 0 on success, <0 on error (-1 invalid argument, -2 launch failure); the message is
 *     available from magpo_last_error() (thread-local).
 *   - "slab" outputs are per-workgroup partial sums [grid][width] that the caller reduces with
 *     magpo_reduce_slabs (fixed order => bit-stable results).
 */
#ifndef MAGPO_H
#define MAGPO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* magpo_stream_t; /* hipStream_t */

const char* magpo_last_error(void);
int magpo_abi_version(void);

/* ---- K12 PRNG: jax.random threefry2x32 (rec_magpo.py:135,202,439,642,660,699; decode.py:141) ---- */
int magpo_threefry_split(const uint32_t* key, uint32_t* out, long num, magpo_stream_t stream);
int magpo_threefry_random_bits(const uint32_t* key, uint32_t* out, long num, magpo_stream_t stream);
int magpo_key_split_host(const uint32_t* key_host, int num, uint32_t* out_host);
int magpo_random_bits_host(const uint32_t* key_host, int num, uint32_t* out_host);
/* jax.random.fold_in(key, data) on the host (flax's per-parameter init keys: rec_magpo.py:598-604,623 via magpo_amd/params.py) */
int magpo_key_fold_in_host(const uint32_t* key_host, uint32_t data, uint32_t* out_host);

/* ---- K1 CoordSum env + wrappers (coordsum/env.py:55-139, wrappers/{matrax,observation,auto_reset_wrapper,episode_metrics}.py) ----
 * The step entry points of all three envs write one TimeStep (mava/types.py:45-123 MarlEnv.step): reward [N][A], discount [N][A]
 * (nullable: the MAGPO learner never reads it), done [N] = timestep.last(), the next observation (the reset observation after an
 * auto-reset), observation.step_count, the action mask where the env has one, and extras["episode_metrics"] (m_ep_ret, m_ep_len,
 * m_term [N]).  Env state is updated in place. */
int magpo_coordsum_reset(int* step_count, int* target, int* record, uint32_t* key, uint32_t* metrics_key,
                         float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A, int K, int TLIM,
                         int maxval, const uint32_t* env_keys, float* obs, int* obs_step, magpo_stream_t stream);
int magpo_coordsum_step(int* step_count, int* target, int* record, uint32_t* key, uint32_t* metrics_key,
                        float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A, int K, int TLIM,
                        int maxval, const int* actions, int act_stride, float* reward, float* discount,
                        unsigned char* done, float* obs, int* obs_step, float* m_ep_ret, int* m_ep_len,
                        unsigned char* m_term, int auto_reset, magpo_stream_t stream);
/* magpo_coordsum_step plus extras["real_next_obs"] (wrappers/auto_reset_wrapper.py:52-83; read by rec_iql.py:254-256): the same kernel, which
 * also writes real_obs [N][A][A + 1] (nullable), the observation of the stepped state BEFORE any auto-reset.  It equals obs on steps
 * without an episode end; every other output and the state are bit-identical to magpo_coordsum_step's. */
int magpo_coordsum_step_real_obs(int* step_count, int* target, int* record, uint32_t* key, uint32_t* metrics_key,
                                 float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A, int K, int TLIM,
                                 int maxval, const int* actions, int act_stride, float* reward, float* discount,
                                 unsigned char* done, float* obs, int* obs_step, float* m_ep_ret, int* m_ep_len,
                                 unsigned char* m_term, int auto_reset, float* real_obs, magpo_stream_t stream);

/* ---- Level-Based Foraging env + wrappers (mava/wrappers/jumanji.py:171-220 LbfWrapper with the always-on team reward, AgentID, AutoReset,
 * RecordEpisodeMetrics; the env itself is jumanji LevelBasedForaging-v0 with RandomGenerator(grid_size, fov, num_agents, num_food,
 * max_agent_level, force_coop), configs/env/scenario/*-coop.yaml).  UNPINNED DYNAMICS: Jumanji's source is not part of the reference tree;
 * csrc/lbf.hip and oracle/lbf.py restate its published algorithm and agree bit for bit with each other.
 * State per env: agent_pos [A][2], agent_level [A], food_pos [NF][2], food_level [NF], food_eaten [NF] u8, step_count, key [2], metrics_key [2],
 * episode-metric counters.  obs [N][A][A + 3 (NF + A)] f32 = [one-hot id | (x, y, level) of foods, self, others], mask [N][A][6] u8. */
int magpo_lbf_reset(int* agent_pos, int* agent_level, int* food_pos, int* food_level, unsigned char* food_eaten,
                    int* step_count, uint32_t* key, uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret,
                    int* ep_len, int N, int A, int NF, int G, int fov, int max_level, int force_coop, int time_limit,
                    const uint32_t* env_keys, float* obs, int* obs_step, unsigned char* mask, magpo_stream_t stream);
int magpo_lbf_step(int* agent_pos, int* agent_level, int* food_pos, int* food_level, unsigned char* food_eaten,
                   int* step_count, uint32_t* key, uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret,
                   int* ep_len, int N, int A, int NF, int G, int fov, int max_level, int force_coop, int time_limit,
                   const int* actions, int act_stride, float* reward, float* discount, unsigned char* done, float* obs,
                   int* obs_step, unsigned char* mask, float* m_ep_ret, int* m_ep_len, unsigned char* m_term,
                   int auto_reset, magpo_stream_t stream);
/* magpo_lbf_step plus extras["real_next_obs"]: the same kernel, which also writes real_obs [N][A][A + 3 (NF + A)] and real_mask [N][A][6],
 * the observation and action mask of the stepped state BEFORE any auto-reset (equal to obs / mask on steps without an episode end).  Both
 * NULL: exactly magpo_lbf_step; one of them NULL is rejected before the launch. */
int magpo_lbf_step_real_obs(int* agent_pos, int* agent_level, int* food_pos, int* food_level, unsigned char* food_eaten,
                            int* step_count, uint32_t* key, uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret,
                            int* ep_len, int N, int A, int NF, int G, int fov, int max_level, int force_coop, int time_limit,
                            const int* actions, int act_stride, float* reward, float* discount, unsigned char* done, float* obs,
                            int* obs_step, unsigned char* mask, float* m_ep_ret, int* m_ep_len, unsigned char* m_term,
                            int auto_reset, float* real_obs, unsigned char* real_mask, magpo_stream_t stream);

/* ---- Robot Warehouse env + wrappers (mava/wrappers/jumanji.py:137-168 RwareWrapper, AgentID, AutoReset, RecordEpisodeMetrics; the env
 * itself is jumanji RobotWarehouse-v0 with RandomGenerator(column_height, shelf_rows, shelf_columns, num_agents, sensor_range,
 * request_queue_size), configs/env/scenario/tiny-4ag.yaml ...).  UNPINNED DYNAMICS like LBF: csrc/rware.hip and oracle/rware.py restate
 * the published algorithm and agree bit for bit.  State per env: grid_a / grid_s [H][W] (agents / shelves layer, 0 = empty, id + 1),
 * agent_pos [A][2], agent_dir [A], agent_carry [A] u8, shelf_req [NS] u8, queue [Q], step_count, amask [A][5] u8, key [2], metrics_key [2],
 * episode-metric counters (H, W, NS from magpo_rware_layout).  obs rows [N][A] of ldo floats = [one-hot id | 8 + 7 (2 r + 1)^2 features]. */
int magpo_rware_layout(int column_height, int shelf_rows, int shelf_columns, int* out);
int magpo_rware_reset(int* grid_a, int* grid_s, int* agent_pos, int* agent_dir, unsigned char* agent_carry,
                      unsigned char* shelf_req, int* queue, int* step_count, unsigned char* amask, uint32_t* key,
                      uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A,
                      int column_height, int shelf_rows, int shelf_columns, int sensor_range, int queue_size,
                      int time_limit, const uint32_t* env_keys, float* obs, long ldo, int* obs_step,
                      unsigned char* mask, magpo_stream_t stream);
int magpo_rware_step(int* grid_a, int* grid_s, int* agent_pos, int* agent_dir, unsigned char* agent_carry,
                     unsigned char* shelf_req, int* queue, int* step_count, unsigned char* amask, uint32_t* key,
                     uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A,
                     int column_height, int shelf_rows, int shelf_columns, int sensor_range, int queue_size,
                     int time_limit, const int* actions, int act_stride, float* reward, float* discount,
                     unsigned char* done, float* obs, long ldo, int* obs_step, unsigned char* mask, float* m_ep_ret, int* m_ep_len,
                     unsigned char* m_term, int auto_reset, magpo_stream_t stream);

/* ---- VectorConnector env + wrappers (mava/wrappers/jumanji.py:223-241,346-455 VectorConnectorWrapper, AgentID, AutoReset,
 * RecordEpisodeMetrics; the env itself is jumanji Connector-v2 with RandomWalkGenerator(grid_size, num_agents), configs/env/scenario/
 * con-*.yaml).  UNPINNED DYNAMICS like LBF / RWARE: csrc/connector.hip and tests/connector_ref.py restate the published algorithm and
 * agree bit for bit.  State per env: grid [G*G] (agent i: path 3i+1, position 3i+2, target 3i+3; empty 0), agent_start / agent_target /
 * agent_pos [A][2] (row, col), step_count, key [2], metrics_key [2], episode-metric counters.  1 <= A <= 32, 2 <= G <= 16.
 * obs rows [N][A] of ldo (>= A + 54) floats = [one-hot id | my_pos / G^2, my_target / G^2, blockers 5x5, targets 5x5]; the floats
 * behind them are not written.  mask [N][A][5] u8 of the state after the step. */
int magpo_connector_reset(int* grid, int* agent_start, int* agent_target, int* agent_pos, int* step_count, uint32_t* key,
                          uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A,
                          int grid_size, int time_limit, const uint32_t* env_keys, float* obs, long ldo, int* obs_step,
                          unsigned char* mask, magpo_stream_t stream);
int magpo_connector_step(int* grid, int* agent_start, int* agent_target, int* agent_pos, int* step_count, uint32_t* key,
                         uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A,
                         int grid_size, int time_limit, const int* actions, int act_stride, float* reward, float* discount,
                         unsigned char* done, float* obs, long ldo, int* obs_step, unsigned char* mask, float* m_ep_ret,
                         int* m_ep_len, unsigned char* m_term, int auto_reset, magpo_stream_t stream);

/* ---- MPE simple_spread env, discrete actions, + wrappers (mava/wrappers/jaxmarl.py:169-243,424-455 MPEWrapper, AgentID, AutoReset,
 * RecordEpisodeMetrics; the env itself is JaxMARL MPE_simple_spread_v3(num_agents, num_landmarks, local_ratio), configs/env/scenario/
 * simple_spread_*.yaml).  UNPINNED DYNAMICS: csrc/mpe.hip and tests/mpe_ref.py restate the published algorithm and agree bit for bit.
 * State per env: pos [A+L][2] f32 (agents, then landmarks), vel [A][2] f32, inner_step (the env's counter), step_count (the wrapper's
 * counter), key [2], metrics_key [2], episode-metric counters.  1 <= A <= 32, 1 <= L <= 32.  obs rows [N][A] of ldo (>= 5 A + 2 L)
 * floats = [one-hot id | vel, pos, landmarks - pos, other agents - pos, comm (zeros)]; the floats behind them are not written.  Every
 * action is legal: no mask.  reward [N][A] per agent; an episode lasts time_limit + 1 steps. */
int magpo_mpe_reset(float* pos, float* vel, int* inner_step, int* step_count, uint32_t* key, uint32_t* metrics_key, float* run_ret,
                    int* run_len, float* ep_ret, int* ep_len, int N, int A, int L, int time_limit, float local_ratio,
                    const uint32_t* env_keys, float* obs, long ldo, int* obs_step, magpo_stream_t stream);
int magpo_mpe_step(float* pos, float* vel, int* inner_step, int* step_count, uint32_t* key, uint32_t* metrics_key, float* run_ret,
                   int* run_len, float* ep_ret, int* ep_len, int N, int A, int L, int time_limit, float local_ratio, const int* actions,
                   int act_stride, float* reward, float* discount, unsigned char* done, float* obs, long ldo, int* obs_step,
                   float* m_ep_ret, int* m_ep_len, unsigned char* m_term, int auto_reset, magpo_stream_t stream);

/* input classes of wrapped CoordSum tokens (first-layer tables, csrc/classtab.hip): cls_enc = ((agent * maxval + target) * npos + pos),
 * cls_dec = prev * npos + pos per row; class_rows writes the distinct rows in class order: obs_tab [A*maxval*npos][A+1], pos_enc,
 * and prev_dec / pos_dec [(K+1)*npos].  The actor's class (agent, target) is cls_enc / npos (or cls_enc itself with pos = NULL, npos = 1;
 * prev / cls_dec may then be NULL as well). */
int magpo_coordsum_classes(const float* obs, int F, const int* prev, const int* pos, int A, int maxval, int npos,
                           int* cls_enc, int* cls_dec, long R, magpo_stream_t stream);
int magpo_coordsum_class_rows(int A, int maxval, int npos, int K, float* obs_tab, int* pos_enc, int* prev_dec, int* pos_dec,
                              magpo_stream_t stream);

/* ---- dense layers on fp32 MFMA (flax nn.Dense / retention projections) ----
 * KIN in {64, 128, 192, 256, 384}.  act: 0 none, 1 relu, 2 gelu(tanh), 3 swish, 4 mask: Y = (M > 0) ? XW+b : 0 with the mask M passed in the
 * mask argument (same stride as Y) -- the ReLU backward fused into dX = dY W^T, 5 tanh, 6 tanh backward: Y = (XW+b) (1 - M^2) with the
 * forward's tanh output M in the mask argument.  mask is an input, required for act 4 / 6 and null otherwise (MAGPO_EINVAL). */
/* variant (any other value is MAGPO_EINVAL): linear 0 = fp32 MFMA, 4 = KIN 128 / 192 with at least 128 output columns (four-wave column
 * blocks) on bf16 MFMA with both operands split into three bf16 pieces (24 mantissa bits, six products, fp32 accumulate: fp32 accuracy
 * at 6/16 of the fp32 MFMA time; ignored for other shapes); wgrad 0 = fp32 MFMA, 64 = 128 x 384 with every row tile full on bf16 MFMA
 * with three-piece operand splits (opt-in: faster, but its accumulation error is ~1.2 x the fp32-MFMA kernel's). */
int magpo_linear(const float* X, int ldx, const float* Wt, const float* bias, float* Y, int ldy, float* mask,
                 long R, int KIN, int NOUT, int act, int variant, magpo_stream_t stream);
int magpo_linear_pro(int pro, const float* a, long lda, const float* y, long ldy_in, const float* s1, const float* s2,
                     const float* pe, const int* pos, long pos_stride, int npos, int use_pe, const float* W,
                     const int* idx, long idx_stride, const float* s_obs, int F, float* out, long ldout,
                     float* outpe, long ldoutpe, const float* Wt, const float* bias, float* Y, long ldy, long R,
                     int NOUT, magpo_stream_t stream);
long magpo_wgrad_workspace_floats(int KIN, int NOUT, int G);
int magpo_wgrad(const float* X, int ldx, const float* dY, int ldy, long R, int KIN, int krows, int NOUT, float* dW,
                float* db, float* workspace, int G, float scale, int accumulate, int variant, magpo_stream_t stream);
/* Backward of a narrow dense layer in one launch: dW[KIN][NOUT] (+ db[NOUT], nullable) = X^T dY and dX[R][KIN] = dY W^T from one pass over
 * X and dY.  KIN in {64, 128}, 1 <= NOUT <= 64; W in its natural [KIN][NOUT] layout (contiguous); ldx, ldy, lddx, ldmask multiples of 4
 * (ldy >= NOUT: columns >= NOUT of dY are never used); X and dY 16-byte aligned (read as float4).  act 0: mask null; act 4: dX = mask > 0 ? dX : 0 (mask [R][KIN], stride ldmask; may
 * be X itself).  dW / db leave as per-workgroup slabs in workspace (>= magpo_wgrad_workspace_floats(KIN, NOUT, G) floats) folded in a fixed
 * order: two launches give the same bits.  Any other argument combination is MAGPO_EINVAL before a pointer is touched. */
int magpo_dense_bwd(const float* X, int ldx, const float* dY, int ldy, const float* W, const float* mask, int ldmask,
                    float* dX, int lddx, long R, int KIN, int NOUT, float* dW, float* db, float* workspace, int G, int act,
                    magpo_stream_t stream);
int magpo_reduce_slabs(const float* slab, float* out, int G, long P, long stride, float scale, int accumulate,
                       magpo_stream_t stream);
int magpo_transpose_pad(const float* W, float* Wt, int K, int N, int Npad, magpo_stream_t stream);
int magpo_small_linear(const float* X, int ldx, int F, const float* W, const float* b, float* Y, int ldy, int N,
                       long R, int relu, magpo_stream_t stream);

/* ---- token-local Sable rows (sable_network.py:62-71,93-137,188-217,255-319; retention.py:289-294) ----
 * E = row width = embed_dim of the device network: 64 (16 lanes x float4 per row) or 128 (32 lanes); slabs are [grid][E]. */
int magpo_row_grid(long R);
int magpo_pe_table(float* pe, int npos, int E, magpo_stream_t stream);
/* embed: z (forward) and z / dz (backward) are nullable -- the backward then recomputes the pre-activation from obs / idx (pass W) */
int magpo_embed_fwd(int mode, const float* obs, int ldo, int F, const float* s_obs, const float* W,
                    const int* idx, int idx_stride, const float* s_ln, const float* pe, const int* pos,
                    int pos_stride, int npos, float* z, int ldz, float* xn, int ldxn, float* kin, int ldkin,
                    long R, int E, magpo_stream_t stream);
int magpo_embed_bwd(int mode, const float* z, int ldz, const float* d0, int ldd0, const float* d1, int ldd1,
                    const float* d2, int ldd2, const float* s_ln, float* dz, int lddz, float* slab_sln,
                    float* slab_w, int nrows, const float* obs, int ldo, int F, const float* s_obs, const float* W,
                    float* slab_sobs, const int* idx, int idx_stride, long R, int E, magpo_stream_t stream);
/* actor MLPTorso layer with LayerNorm (torsos.py:36-47): y = act(LayerNorm(z) + b) over rows of D floats, D in {64, 128, 192, 256};
 * LayerNorm(use_scale=False): (z - mean) rstd, rstd = rsqrt(max(E[z^2] - E[z]^2, 0) + 1e-6); act 0 none, 1 relu, 5 tanh (magpo_linear's codes).
 * fwd writes y, xhat = (z - mean) rstd and rstd [R]; bwd: g = dy act'(y), dz = rstd (g - mean(g) - xhat mean(g xhat)), slab_b
 * [magpo_row_grid(R)][D] = per-workgroup column sums of g (the bias gradient, for magpo_reduce_slabs).  Strides multiples of 4. */
int magpo_ln_act_fwd(const float* z, int ldz, const float* bias, float* y, int ldy, float* xhat, int ldxh, float* rstd, long R, int D,
                     int act, magpo_stream_t stream);
int magpo_ln_act_bwd(const float* dy, int lddy, const float* y, int ldy, const float* xhat, int ldxh, const float* rstd, float* dz,
                     int lddz, float* slab_b, long R, int D, int act, magpo_stream_t stream);
int magpo_small_relu_wgrad(const float* X, int ldx, int F, const float* Yact, const float* dY, float* slab_w, long R,
                           magpo_stream_t stream);
int magpo_small_operand(int mode, const float* obs, int ldo, int F, const float* s_obs, const int* idx,
                        int idx_stride, float* out, long R, magpo_stream_t stream);
int magpo_retpost_fwd(const float* r, int ldr, const float* gp, int ldg, const float* gamma, const float* beta,
                      float* u, int ldu, long R, int hs, int gs, int E, magpo_stream_t stream);
int magpo_retpost_bwd(const float* r, int ldr, const float* gp, int ldg, const float* gamma, const float* beta,
                      const float* du, int lddu, float* dr, int lddr, float* dgp, int lddg, float* slab_gamma,
                      float* slab_beta, long R, int hs, int gs, int E, magpo_stream_t stream);
int magpo_resnorm_fwd(const float* a, int lda, const float* y, int ldy, const float* s1, const float* s2,
                      const float* pe, const int* pos, int pos_stride, int npos, float* out, int ldout,
                      float* outpe, int ldoutpe, long R, int E, magpo_stream_t stream);
int magpo_resnorm_bwd(const float* a, int lda, const float* y, int ldy, const float* s1, const float* s2,
                      const float* d0, int ldd0, const float* d1, int ldd1, const float* d2, int ldd2,
                      float* dsum, int lddsum, float* slab_s1, float* slab_s2, long R, int E, magpo_stream_t stream);
/* residual + flax nn.LayerNorm (mat_network.py:65-66,80,85,99,108,135-137,197): out = LayerNorm(x) * scale + bias over rows of E floats,
 * epsilon 1e-6; x = a + y (a nullable: plain LayerNorm of y) with act 0, x = gelu(y) (tanh form; a must be null) with act 2.  The
 * statistics run over the first nf columns (1 <= nf <= E; the columns beyond are read as zero and leave as bias: a LayerNorm over nf raw
 * features inside a zero-padded row; scale and bias always hold E floats).  bwd recomputes the statistics: dsum = d(a + y) (act 2: dy)
 * of the incoming d0 [+ d1], slab_scale / slab_bias [magpo_row_grid(R)][E] = per-workgroup column sums of d * xhat / d (for
 * magpo_reduce_slabs).  Strides multiples of 4 and >= E.  gelu_bwd: dz = dy gelu'(z) on rows of E floats. */
int magpo_resln_fwd(const float* a, int lda, const float* y, int ldy, const float* scale, const float* bias, float* out, int ldout,
                    long R, int E, int nf, int act, magpo_stream_t stream);
int magpo_resln_bwd(const float* a, int lda, const float* y, int ldy, const float* scale, const float* d0, int ldd0, const float* d1,
                    int ldd1, float* dsum, int lddsum, float* slab_scale, float* slab_bias, long R, int E, int nf, int act,
                    magpo_stream_t stream);
int magpo_gelu_bwd(const float* z, int ldz, const float* dy, int lddy, float* dz, int lddz, long R, int E, magpo_stream_t stream);
int magpo_headmid_fwd(const float* hpre, int ldh, const float* s, float* hn, int ldhn, const float* w,
                      const float* b, float* value, int value_stride, long R, int E, magpo_stream_t stream);
int magpo_headmid_bwd(const float* hpre, int ldh, const float* s, const float* dhn, int lddhn, const float* w,
                      const float* dvalue, int dvalue_stride, float* dhpre, int lddh, float* slab_s,
                      float* slab_w, float* slab_b, long R, int E, magpo_stream_t stream);
/* wide observations (obs_dim > 32: rows padded to 128 columns, first layers on the MFMA dense kernels; csrc/wideobs.hip):
 * on = RMSNorm_F(obs) * s_obs (sable_network.py:93-95), its s_obs gradient as [magpo_obsnorm_grid(R)][128] slabs, and x + pe[pos] */
int magpo_obsnorm_grid(long R);
int magpo_obsnorm_fwd(const float* obs, long ldo, int F, const float* s_obs, float* on, long R, magpo_stream_t stream);
int magpo_obsnorm_bwd(const float* obs, long ldo, int F, const float* don, float* slab_s, long R, magpo_stream_t stream);
int magpo_add_pe(const float* x, long ldx, const float* pe, const int* pos, long pos_stride, int npos, float* out,
                 long ldout, long R, int E, magpo_stream_t stream);
int magpo_relu_bwd(const float* act, const float* dy, float* dx, long n, magpo_stream_t stream);
int magpo_add_inplace(float* dst, const float* src, long n, magpo_stream_t stream);
/* dst[r][0..W) += src[r][0..W) over R rows (row strides ldd / lds): the partial sums of the blockwise 128-wide retention head */
int magpo_add_rows(float* dst, long ldd, const float* src, long lds, long R, int W, magpo_stream_t stream);

/* ---- K2/K7 retention (retention.py:66-115 chunkwise + recurrent, :117-213 decay matrix / xi) ---- */
/* qkv_rows (nullable): q | k | v are row tables (block-0 projections exist once per distinct input row, csrc/classtab.hip) and token row r
 * reads table row qkv_rows[r]; r, dr, dq, dk, dv are always per token row. */
/* chunk_tokens: tokens per chunk of the chunkwise kernels, 32 (= 0, the default: two workgroups per CU, less masked work; teams of more than 32
 * agents fall back to 64) or 64.  The forward (saved chunk-entry states [nseq][num_chunks][64][64]) and the backward of one pass must be given
 * the same value, and so must magpo_retention_num_chunks when it sizes `states`. */
int magpo_retention_num_chunks(int T, int A, int chunk_tokens);
int magpo_retention_chunk_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                              float* r, long ldr, const float* s0, const int* seq_env,
                              const unsigned char* dones, float* states, float* s_final, int nseq, int T, int A,
                              int masked, float kappa, int hs, const int* qkv_rows, int chunk_tokens, magpo_stream_t stream);
int magpo_retention_chunk_bwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                              const float* dr, long lddr, float* dq, long lddq, float* dk, long lddk, float* dv,
                              long lddv, const unsigned char* dones, const float* states, int nseq, int T, int A,
                              int masked, float kappa, int hs, const int* qkv_rows, int chunk_tokens, magpo_stream_t stream);
/* recurrent form (acting): ntok tokens per env, 1 <= ntok <= 32 (up to 16 staged in 28 KiB of LDS, 17 - 32 in 56 KiB). */
int magpo_retention_recurrent(float* S, const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                              long env_stride_rows, float* r, long ldr, int nenv, int ntok, int ret_from, float decay,
                              int write_state, const float* gp, long ldg, const float* gamma, const float* beta,
                              int hs, int gs, magpo_stream_t stream);
int magpo_zero_states_where_done(float* s0, float* s1, float* s2, const unsigned char* done, int nenv,
                                 magpo_stream_t stream);
/* stateless retention over nteams independent teams of A consecutive token rows (retention.py:79-84, 94-99 with memory_config.type
 * "ff_sable" on a zero hidden state; csrc/team_retention.hip): r_i = sum_j M_ij (q_i . k_j) v_j over the rows i, j of one team, M_ij = [j <= i]
 * when masked, else 1.  No decay, no carried state: nothing is read but the operands and nothing is written but r (dq | dk | dv).
 * 1 <= A <= 32; hs = tile width in 1..64 (a head, or one 64-wide block of a wider head: the masked product is linear in the q / k blocks);
 * row strides multiples of 4 floats.  ntok / ret_from as in magpo_retention_recurrent: only rows ret_from <= i < ntok of every team are
 * produced, from the k / v rows j < ntok (training: ntok = A, ret_from = 0; decoder iteration i of acting: ntok = i + 1, ret_from = i).
 * gp (nullable) selects magpo_retention_recurrent's fused GroupNorm + swish-gate epilogue, with the same gamma / beta / gs contract.
 * bwd: dP = (dr v^T) * M, dq = dP k, dk = dP^T q, dv = ((q k^T) * M)^T dr, every row of every team. */
int magpo_team_retention_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* r, long ldr,
                             long nteams, int A, int ntok, int ret_from, int masked, int hs, const float* gp, long ldg,
                             const float* gamma, const float* beta, int gs, magpo_stream_t stream);
int magpo_team_retention_bwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* dr, long lddr,
                             float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, long nteams, int A, int masked,
                             int hs, magpo_stream_t stream);

/* ---- softmax attention over independent teams (attention.py:50-77 between the projections): the Multi-Agent Transformer ----
 * The team layout of magpo_team_retention_*: nteams teams of A consecutive token rows (1 <= A <= 32); one thread per (team, row, head),
 * sums in fp64 on the vector ALU and one fp32 rounding per output; nh heads of hs in {16, 32, 64} channels, head n at columns n hs .. of
 * the q / k / v / y rows; q, k, v separate pointers with their own row strides (multiples of 4 floats, >= nh hs).  P = softmax_j((q_i . k_j) / sqrt(hs) + mask), y = P v, masked: j <= i
 * only (masked pairs weigh exactly 0; the row maximum is subtracted).  ntok / ret_from as above: only rows ret_from <= i < ntok are
 * produced, from the k / v rows j < ntok.  fwd also writes lse [R][nh] = log sum_j exp(s_ij) for the rows it produces.
 * bwd recomputes P from q, k and lse (no [A][A] matrix in memory): dv = P^T dy, dS = P o (dy v^T - rowsum(P o dy v^T)) (the row sum
 * equals rowsum(dy o y)), dq = dS k / sqrt(hs), dk = dS^T q / sqrt(hs), every row of every team. */
int magpo_team_attention_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* y, long ldy,
                             float* lse, long nteams, int A, int ntok, int ret_from, int masked, int hs, int nh, magpo_stream_t stream);
int magpo_team_attention_bwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* lse,
                             const float* dy, long lddy, float* dq, long lddq, float* dk, long lddk, float* dv, long lddv,
                             long nteams, int A, int masked, int hs, int nh, magpo_stream_t stream);

/* ---- K2 fused acting step: SableNetwork.get_actions (sable_network.py:443-482; decode.py:111-153) in ONE launch ----
 * dims_host[16] = {N, A, K, F, n_block, n_head, hs, gs, npos, value_only, obs row stride (>= F), envs per wave (0 = by size, or 4 / 8 / 16),
 *   pending, flush, precand, defer}; kappa_host[4] (per head);
 * keys_host [A][2] sampling keys by value, or NULL with ptrs[3] = device key table (static arguments for graph replay);
 * Decoder states are read once and written once per step: the update S <- kappa S + sum_a k_a^T v_a of a step is DEFERRED to the next launch
 *   (the step's k | v rows stay in the scratch rows qkvg1 / kvg2, which therefore must persist between the launches of a rollout).
 *   pending = 1: the previous launch left such rows (apply them first); flush = 1: also apply this launch's rows before returning (with
 *   value_only: the pending ones), so that S_d1 / S_d2 hold the carried states again.  A stand-alone step is {pending 0, flush 1}; a rollout is
 *   {0, 0}, {1, 0} ... and ends with a launch that has flush = 1 (e.g. the bootstrap-value launch {value_only 1, pending 1, flush 1}).
 * defer = 1 (env-step launches of a rollout; excludes flush / value_only): with one head, every other group of workgroups runs the block-0
 *   candidate pre-pass of the NEXT step at the end of this launch (S_d1 of their envs then already holds this step's rows; their candidate
 *   table assumes step count + 1 and no episode end); precand = 1 tells the next launch (same N, same envs per wave) that this happened: those
 *   workgroups skip the pre-pass, zero state and table where `done` says the episode ended, and a flushing launch leaves their S_d1 alone.  A
 *   rollout is {pending, precand, defer, flush} = {0,0,1,0}, {1,1,1,0} ... and ends with the value launch {1,1,0,1}; a stand-alone step is
 *   {0,0,0,1}.  Purpose: these workgroups stream states while the others decode (the launch alternates HBM-bound and dense phases).
 * ptrs_host[49]: obs pos mask keys_dev | s_obs W_obs s_encln W_act s_decln | vh0_t vh0_b vh_s vh_w vh_b1 | h0_t h0_b h_s h1_t h1_b |
 *   pe | S_enc S_d1 S_d2 ([n_block][n_head][N][64][64], updated in place) | scratch xn ([N*A] rows), done [N] u8 or NULL (envs whose
 *   episode just ended: their carried states read as zero, rec_magpo.py:164-169), scratch qkvg u y rep reppe hv ([N*A] rows) |
 *   xa kin1 y1 c cpe y2 xo xope hp hn logits ([N] rows) | u1 u2 ([N*A] rows) | prev [N][A] i32 | action [N][A] i32, logp, value [N][A] |
 *   ptab [N][K + 2][64] scratch (n_head = 1: block-0 self-retention candidate table);
 * blk_ptrs_host[21 * n_block]: qkvg_t wo_t ln1 ln2 gn_g gn_b | qkvg1_t wo1_t dln1 gn1_g gn1_b | q2_t kvg2_t wo2_t dln2 dln3 gn2_g gn2_b |
 *   scratch qkvg1 [N*A][256], q2 [N*A][64], kvg2 [N*A][256] (rows [k | v | - | q2 (kappa S)]).
 *   *_t = the transposed weights of magpo_transpose_pad in the FRAGMENT-MAJOR layout of magpo_act_weight_layout (below): a wave streams
 *   its weight fragments from L2 for every token, and one fragment load must be 1 KB contiguous for that stream to run at the L1 rate. */
int magpo_sable_act(const int* dims_host, const float* kappa_host, const uint32_t* keys_host, const void* const* ptrs_host,
                    int nptrs, const void* const* blk_ptrs_host, int nblk_ptrs, magpo_stream_t stream);
/* Wf[g][gk][lane = m + 16 kq][c] = Wt[16 g + m][16 gk + 4 kq + c] for a transposed weight Wt [nrows][64] (nrows a multiple of 16):
 * the weight operand layout of magpo_sable_act.  Rebuilt by the host after every parameter update (SableGuider.build_act_weights). */
int magpo_act_weight_layout(const float* Wt, float* Wf, int nrows, magpo_stream_t stream);
/* Envs per wave (4, 8 or 16) of the launch magpo_sable_act makes for N envs of A agents; forced = dims_host[11] (0 = chosen by size).
 * The kernel instance is k_sable_act<envs per wave, A <= 4 ? 4 : 8, (n_head == 1 && A <= 4) ? 1 : 0>.  Returns -1 for an invalid `forced`.
 * Shape limits of magpo_sable_act: 1 <= A <= 8, n_block <= 4, n_head in {1, 2, 4}, K <= 31 (the candidate pre-pass holds K + 2 <= 48 rows). */
int magpo_sable_act_envs_per_wave(int N, int A, int forced);

/* ---- fused training-forward segment between two retention ops (sable_network.py:62-71,188-217,277-319; retention.py:289-295; n_head = 1):
 *   u = swish(g) * GroupNorm(r) ; y = u W_o ; o = rms(res + y) s1 [-> rms s2] ; ope = o + pe[pos] ; then the tail
 *   tail 1 (encoder): hv = o W0 + b0, value = rms(gelu(hv)) hs . hw + hb1, q2[k] = ope Wq2[k]   tail 2: out0 = ope W0 (192 columns)
 *   tail 3 (last decoder block): hp = o W0 + b0, hn = rms(gelu(hp)) hs, logits = hn W1 + b1 (K columns)   tail 0: none
 * dims_host[6] = {tail, K, npos, ldg, ld0, nq2}; ptrs_host[34] (device pointers): r gp gamma beta wo_t res s1 s2 pe pos | u y o ope |
 *   w0_t b0 out0 | hs hw hb1 value | q2_t[4] q2[4] | hn w1_t b1 logits | rows   (u, y, o, ope, s2, rows and unused tail pointers may be NULL;
 *   with rows (i32 [R]) gp and res are row tables and token row r reads table row rows[r]) */
int magpo_seg_post(const int* dims_host, long R, const void* const* ptrs_host, int nptrs, magpo_stream_t stream);

/* backward of that front: dsum = d(res + y) through the RMSNorm(s), du = dsum W_o^T, (dr, dg) through GroupNorm + swish gate, and the
 * parameter-gradient rows (s1, s2, gamma, beta) as [magpo_seg_bwd_grid(R)][64] slabs.  ptrs_host[21]: a y s1 s2 d0 d1 d2 wo_nat r gp gamma beta |
 * dsum dr dgp | slab_s1 slab_s2 slab_ga slab_be | rows | wo_t   (y, s2, d1, d2, slab_s2, rows, wo_t may be NULL; with rows, a and gp are row
 * tables; with wo_t -- W_o^T as magpo_seg_post takes it -- y is not read but recomputed from r and gp, and magpo_seg_post may be given y = NULL)
 * ptrs_host[22]: the same 21 slots + slot 21 = slab_wo (may be NULL; needs wo_t): [magpo_seg_bwd_grid(R)][64 * 64] fp32, each workgroup's partial
 * sum of dW_o = u^T dsum in the natural [in][out] order of W_o, folded by magpo_reduce_slabs(slab_wo, dW_o, grid, 4096, 4096, ...).  With it
 * magpo_seg_post may be given u = NULL as well: nothing else reads u.  Any other table size, or slab_wo without wo_t, is MAGPO_EINVAL. */
int magpo_seg_bwd_grid(long R);
int magpo_seg_bwd(long R, long ldg, long lddg, const void* const* ptrs_host, int nptrs, magpo_stream_t stream);

/* ---- K3/K8 GRU actor (base.py:121-184; flax GRUCell) ----
 * gates [R][512] is an opaque save-for-backward buffer written by magpo_gru_scan_fwd and read by magpo_gru_scan_bwd
 * ((r, z, n, h W_hn + b_hn) interleaved per hidden column).
 * Per-call tuning: split_bf16 -- the TRAINING scans (T > 1 with all save buffers) on 0 = fp32 MFMA; 1 = bf16 pairs (x = hi + lo, product =
 * hi*hi + hi*lo + lo*hi with fp32 accumulation, ~2^-16 relative per product; forward and backward); 2 = bf16 triples (x = hi + mid + lo: the 24
 * mantissa bits of an fp32 operand, six products hh hm mh hl lh mm = 6/16 of the fp32 MFMA time at fp32 accuracy; forward scan, the backward --
 * bound by its gate / gradient traffic -- stays on fp32 MFMA).  Forward and backward of one pass take the same value.  block_rows -- recurrent rows per workgroup of the fp32 scans: 0 = by size (32 when 64-row blocks would leave half of the compute
 * units idle), or 32 / 64 forced.
 * xi_cls (nullable): xi is a table over the distinct input rows and token row r takes xi[xi_cls[r]] (csrc/classtab.hip). */
int magpo_gru_scan_fwd(const float* xi, const float* Wht, const float* b_hn, const float* h0, const int* h0_idx,
                       const unsigned char* reset, float* hs, float* gates, float* hprev, int nseq, int T, int A,
                       const int* xi_cls, int split_bf16, int block_rows, magpo_stream_t stream);
/* hidden-state carry over a TIME-MAJOR trajectory: xi rows (t, env, agent), reset_tm [T][nenv]; writes only the state after step T-1 */
int magpo_gru_carry(const float* xi, const float* Wht, const float* b_hn, const float* h0, const unsigned char* reset_tm,
                    float* h_last, int nenv, int T, int A, const int* xi_cls, int block_rows, magpo_stream_t stream);
/* backward scan.  dg [R][512] = the gate pre-activation gradients of every token row as ONE matrix (dn_in | dr | dz | dn_hid): the
 * gradient of the input projection xi = (r | z | n) is its columns (128..383 | 0..127) and that of the hidden projection h W_h its columns
 * 128..511 (dr and dz are shared by the two sides and written once; ld 512 either way).  slab_bhn [ceil(nseq A / 64)][128]: per-block
 * column sums of dn_hid (the b_hn gradient, folded by magpo_reduce_slabs). */
int magpo_gru_scan_bwd(const float* gates, const float* hprev, const unsigned char* reset, const float* dhs,
                       const float* Wh, float* dg, float* slab_bhn, int nseq, int T, int A,
                       int split_bf16, int block_rows, magpo_stream_t stream);
/* ONE GRU cell step, for one or two networks in a single launch (csrc/gru_step.hip; the acting step of recurrent PPO, rec_mappo.py:96-141):
 * h_out = GRUCell(h_in zeroed where reset, emb), the recurrence above with the input projection emb W_i + b_i formed inside the kernel (no xi
 * buffer).  dims_host[3] = {nnets (1 or 2), D of network 0, D of network 1}; D = width of emb, 64 / 128 / 192 / 256, and may differ between the
 * networks.  ptrs_host[7 nnets] (device pointers), per network: emb [R][D], Wit [384][D], bi [384], Wht [384][128], b_hn [128], h_in [R][128],
 * h_out [R][128] (Wit / Wht as magpo_transpose_pad writes them; h_out may be h_in).  reset [ceil(R / A)] u8: row r belongs to env r / A.
 * Grid (ceil(R / 64), nnets); rows beyond R are never written.  Rejected before any launch: R < 1, A < 1, nnets not 1 or 2, nptrs != 7 nnets,
 * a D outside the set, a null pointer. */
int magpo_gru_cell_step(const int* dims_host, const void* const* ptrs_host, int nptrs, const unsigned char* reset, int R,
                        int A, magpo_stream_t stream);
/* ONE acting step of feed-forward PPO, for one or two networks in a single launch (csrc/mlp_step.hip; ff_mappo.py:75-100):
 * Y = head(MLPTorso(X)) on R rows, per layer Dense -> activation (no LayerNorm), then Dense(NOUT) without activation; the hidden activations
 * stay in LDS.  The networks of one launch may differ in everything below.
 *   dims_host[1 + 10 nnets] = {nnets (1 or 2); per network: F, ldx, layers, width 0, width 1, width 2, activation, activate_final, NOUT, ldy}
 *     F features per row, 1..128, rows ldx >= F floats apart (any ldx: a row need not be 16-byte aligned; columns >= F are never read);
 *     1..3 layers, every used width 64 / 128 / 192 / 256 (unused width slots are ignored); activation 1 relu / 5 tanh as magpo_linear,
 *     applied to every layer but the last, and to the last when activate_final is 1; NOUT 1..32, output rows ldy >= NOUT floats apart.
 *   ptrs_host[10 nnets] (device pointers), per network: X, W0, b0, W1, b1, W2, b2, Wh, bh, Y (slots of unused layers may be null)
 *     Wi, i > 0: [width i][width i-1], the transposed layout magpo_transpose_pad writes; Wh: [>= 32][last width] likewise (rows >= NOUT are
 *     read, never used); bi [width i], bh [NOUT].
 *     W0: when F <= 32, width 0 = 128 and layer 0 is followed by relu -- the first layer magpo_small_linear serves -- the NATURAL [F][128]
 *     kernel, summed as that kernel sums it; otherwise the transposed [width 0][KP], KP = 64 for F <= 32, else 128, with zero columns >= F.
 * Writes exactly columns 0 .. NOUT-1 of rows 0 .. R-1 of each Y (NOUT = 1, ldy = 1: a value vector).  Grid (ceil(R / 64), nnets).
 * Rejected before any launch: R < 1, nnets not 1 or 2, nptrs != 10 nnets, layers outside 1..3, a used width outside the set, F, ldx, NOUT or
 * ldy out of range, an unknown activation code, activate_final not 0 / 1, a null pointer in a used slot. */
int magpo_mlp_act_step(const int* dims_host, const void* const* ptrs_host, int nptrs, int R, magpo_stream_t stream);
/* ONE acting step of the memoryless Sable (ff_sable) in a single launch (csrc/ff_sable_act.hip; SableGuider.act with memory_type "ff_sable":
 * sable_network.py:443-482, decode.py:111-153 on zero hidden states): encoder over the A tokens of the step, value head, the A autoregressive
 * decoder iterations with self- and cross-retention over the step's own tokens j <= i, logit head, masked log-softmax and Gumbel-argmax with the
 * counter layout of magpo_sample_categorical (counter n K + k of agent i's key).  Stateless: kappa = 1 and a zero positional-encoding table are
 * assumed (the caller checks both), nothing is carried between calls.  A workgroup owns 32 envs; grid ceil(N / 32).
 *   dims_host[10] = {N, A, K, F, n_block, n_head, hs, gs, value_only, obs_ld}: 64-wide rows, hs = 64 / n_head, gs = hs / n_head; obs rows of
 *     F features obs_ld >= F floats apart (any obs_ld; columns >= F are never read).  value_only = 1 writes value_out and nothing else.
 *   keys_host [A][2] (agent i samples from key i), or NULL: then ptrs_host[2] is the device key table [A][2] (static arguments for graph replay).
 *   ptrs_host[22] (device pointers):
 *      0 obs [N][A][obs_ld]            1 mask [N][A][K] u8 (nullable)       2 keys_dev [A][2] u32 (nullable)
 *      3 enc.obs.norm.scale [F]        4 enc.obs.dense.kernel [F][64]       5 enc.ln.scale [64]
 *      6 dec.act.kernel [K + 1][64]    7 dec.ln.scale [64]
 *      8 enc.head.dense0 Wt [64][64]   9 enc.head.dense0.bias [64]         10 enc.head.norm.scale [64]
 *     11 enc.head.dense1.kernel [64]  12 enc.head.dense1.bias [1]
 *     13 dec.head.dense0 Wt [64][64]  14 dec.head.dense0.bias [64]         15 dec.head.norm.scale [64]
 *     16 dec.head.dense1 Wt [>= 32][64] (rows >= K zero)                   17 dec.head.dense1.bias [K]
 *     18 scratch [scratch_floats]     19 action_out [N][A] i32             20 logp_out [N][A]         21 value_out [N][A]
 *     (19, 20 may be null with value_only = 1)
 *   blk_ptrs_host[18 n_block], per block (Wt = the transposed [out][64] layout magpo_transpose_pad writes):
 *      0 enc retn.w_qkvg Wt [256][64]  1 enc retn.w_o Wt [64][64]   2 enc ln1.scale   3 enc ln2.scale   4 enc retn.gn.scale [hs]   5 enc retn.gn.bias [hs]
 *      6 dec retn1.w_qkvg Wt [256][64] 7 dec retn1.w_o Wt [64][64]  8 dec ln1.scale   9 dec retn1.gn.scale [hs]  10 dec retn1.gn.bias [hs]
 *     11 dec retn2.w_q Wt [64][64]    12 dec retn2.w_kvg Wt [192][64]  13 dec retn2.w_o Wt [64][64]  14 dec ln2.scale  15 dec ln3.scale
 *     16 dec retn2.gn.scale [hs]      17 dec retn2.gn.bias [hs]
 *   scratch: at least 32 ceil(N / 32) A (384 + 256 n_block) floats, 16-byte aligned, from the caller's workspace (never allocated inside the call);
 *     every workgroup writes and reads only its own tile's rows.  Contents on return are unspecified.
 * Writes exactly rows 0 .. N-1 of the outputs.  No atomics: equal inputs give identical bits.  Rejected before any launch: N < 1, A outside 1..8,
 * n_block outside 1..4, n_head not 1 / 2 / 4 or hs / gs inconsistent with it, K outside 1..31, F outside 1..128, obs_ld < F, table sizes other than
 * 22 / 18 n_block, a null pointer in a required slot, no keys without value_only, scratch_floats too small. */
int magpo_ff_sable_act(const int* dims_host, const uint32_t* keys_host, const void* const* ptrs_host, int nptrs,
                       const void* const* blk_ptrs_host, int nblk_ptrs, long scratch_floats, magpo_stream_t stream);
/* observation.global_state of the centralised critic (mava/wrappers/matrax.py:128-131, jumanji.py:61-67): out [N A][ld], row (n, a) = the
 * concatenation over agents j of obs[(n, j)][id_cols .. id_cols + F_raw) (the raw agent views behind the id_cols leading agent-id columns of the
 * stored rows, row stride ldo), the same for every a, zero from column A F_raw to ld.  ld is 64 or 128 and A F_raw <= ld. */
int magpo_global_state(const float* obs, long ldo, int id_cols, int F_raw, float* out, int ld, int N, int A,
                       magpo_stream_t stream);

/* ---- K2 sampling, K5 GAE, K6 shuffle/layout, K9 losses (decode.py:128-149; multistep.py:24-68; rec_magpo.py:222-370,439-462) ---- */
int magpo_sample_categorical(const float* logits, long ld, const unsigned char* mask, long mask_stride,
                             uint32_t k0, uint32_t k1, const uint32_t* key_dev, int* action, long act_stride, float* logp,
                             long logp_stride, int* next_idx, long next_stride, float* lp_all, long lp_ld, int N,
                             int K, magpo_stream_t stream);
/* GAE (multistep.py:24-68): done [T][N] with done[t] = "the observation of step t starts an episode", last_done [N] the same for step T.
 * N * A < 8192 sequences (and T >= 16): a wavefront prefix scan over time, one wave per (env, agent) sequence (log-depth instead of T
 * dependent steps); otherwise one thread per sequence, coalesced across sequences.  Same recurrence, fp32 summation order differs. */
int magpo_gae(const float* reward, const float* value, const unsigned char* done, const float* last_val,
              const unsigned char* last_done, float* adv, float* targets, int T, int N, int A, float gamma,
              float lam, magpo_stream_t stream);
/* o_h0idx [mb][A] (nullable): row env * A + agent of every gathered sequence's start state, which only the GRU actor reads. */
int magpo_gather_minibatch(const float* obs, const int* action, const int* stepcount, const unsigned char* done,
                           const unsigned char* mask, const float* value, const float* logp, const float* adv,
                           const float* targets, const int* env_idx, const int* agent_perm, float* o_obs,
                           int* o_action, int* o_prev, int* o_pos, unsigned char* o_done, unsigned char* o_mask,
                           float* o_value, float* o_logp, float* o_adv, float* o_targets, int* o_h0idx, int T,
                           int N, int A, int F, int K, int mb, magpo_stream_t stream);
/* ---- input-class tables (csrc/classtab.hip): a first layer applied to R rows that take only C << R distinct values is the layer
 * applied to the C distinct rows + a row gather; its parameter gradient is the layer's backward on per-class sums of dY.
 * (mava/networks/base.py:166-170 pre-torso + GRU input projection; sable_network.py:93-101,257-267 obs / action embeddings)
 * class_sum: order [R] = row ids sorted stably by class, offsets [C+1] = class boundaries in order (both int64, device);
 * partial [magpo_class_sum_slots(C)][C][W] workspace; out [C][W].  Bit-stable (data-dependent order only). */
int magpo_gather_rows(const float* table, long ldt, const int* cls, float* out, long ldo, long R, int W,
                      magpo_stream_t stream);
int magpo_class_sum_slots(int C);
int magpo_class_sum(const float* X, long ldx, const long* order, const long* offsets, int C, int W, float* partial,
                    float* out, magpo_stream_t stream);
int magpo_adv_moments(const float* x, long n, double* workspace, float* out, magpo_stream_t stream);
int magpo_loss_fwd_bwd(const float* g_logits, long ldg, const float* a_logits, long lda, const unsigned char* mask,
                       const int* action, const float* old_logp, const float* old_value, const float* value,
                       const float* adv, const float* targets, const float* adv_stats, float* dg_logits,
                       long lddg, float* da_logits, long lddda, float* dvalue, double* workspace, float* loss_out,
                       long R, int K, float clip_eps, float clip_gpo, float ent_coef, float vf_coef, float alpha,
                       magpo_stream_t stream);
/* PPO loss of the guider-only system (rec_sable.py:177-226): the guider half of magpo_loss_fwd_bwd without an actor.  Same contracts as
 * dg_logits there: columns K .. min(lddl, 64) and illegal columns exactly 0, a row with one legal action has no gradient, input columns
 * >= K are loaded and discarded, two-stage reduction in a fixed order (bit-stable), workspace >= 8 * 1024 doubles.
 * loss_out [4] = [total, actor_loss, entropy, value_loss], total = actor - ent_coef entropy + vf_coef value; dlogits / dvalue = d total.
 * Rejected before any launch: R < 1, K > 64, K > ld, K > lddl, lddl not a multiple of 4. */
int magpo_ppo_loss_fwd_bwd(const float* logits, long ld, const unsigned char* mask, const int* action,
                           const float* old_logp, const float* old_value, const float* value, const float* adv,
                           const float* targets, const float* adv_stats, float* dlogits, long lddl, float* dvalue,
                           double* workspace, float* loss_out, long R, int K, float clip_eps, float ent_coef,
                           float vf_coef, magpo_stream_t stream);
int magpo_copy_rows(const float* src, long lds_, float* dst, long ldd, long R, int W, magpo_stream_t stream);

/* ---- Q-learning (csrc/qlearn.hip; mava/systems/q_learning/anakin/rec_iql.py:210-401, networks/distributions.py:94-138) ----
 * Shared contracts: no hidden state, arguments validated before any launch, no atomics, equal inputs give equal bits, and whatever changes
 * from env step to env step (key, env-step counter, ring cursor) is read from device memory so that a captured rollout replays.
 * UNPINNED: tfp's Categorical(probs).sample, flashbax's trajectory buffer and optax's target updates are not in the reference tree; these
 * entry points agree bit for bit with their restatement in tests/iql_ref.py.
 *
 * MaskedEpsGreedyDistribution(q, eps, mask).sample, one row per (env, agent): q [R][ld] with K <= 32 valid columns, mask [R][K] u8
 * (nullable = all legal; a row needs one legal action), key = (k0, k1) or key_dev (device, overrides).  eps = max(eps_min, 1 - (t / eps_decay)
 * * (1 - eps_min)) in fp32 in that order with t = t_dev[0]; t_dev NULL = eps 0.  probs = eps * mask / n_avail + (1 - eps) * onehot(greedy),
 * greedy = argmax of q over the legal actions (first maximum); action = argmax_k(log(probs_k) + gumbel(counter r K + k)), the log rounded
 * once from double like the gumbel.  With eps = 0 action = greedy whatever the key.  action [R] i32; greedy [R] i32 nullable.
 * Rejected: K < 1, K > 32, ld < K, R K >= 2^32, NULL q / action, and (with t_dev) eps_decay <= 0 or eps_min outside [0, 1]. */
int magpo_eps_greedy_sample(const float* q, long ld, const unsigned char* mask, uint32_t k0, uint32_t k1,
                            const uint32_t* key_dev, const int* t_dev, float eps_min, float eps_decay, int* action,
                            int* greedy, long R, int K, magpo_stream_t stream);
/* Trajectory ring of one group: every field is a time ring [N][S] (S = buffer_size): r_obs / r_next_obs [N][S][A][F] dense rows,
 * r_mask / r_next_mask [N][S][A][K] u8 (both NULL for envs without masks), r_action i32 / r_reward f32 [N][S][A], r_terminal / r_tot
 * (term_or_trunc) [N][S] u8.  magpo_replay_add copies one env step (obs rows with stride ldo, next_obs rows = real_next_obs with stride
 * ldn, mask / next_mask [N][A][K], action / reward [N][A], terminal / tot [N]) into slot cursor[0] of every env, then a second one-thread
 * launch sets cursor = (cursor + 1) % S and filled = min(filled + 1, S) (device ints, plain stores).  A cursor outside [0, S) is clamped. */
int magpo_replay_add(float* r_obs, unsigned char* r_mask, int* r_action, float* r_reward, unsigned char* r_terminal,
                     unsigned char* r_tot, float* r_next_obs, unsigned char* r_next_mask, int* cursor, int* filled, int N,
                     int S, int A, int F, int K, const float* obs, long ldo, const unsigned char* mask, const int* action,
                     const float* reward, const unsigned char* terminal, const unsigned char* tot, const float* next_obs,
                     long ldn, const unsigned char* next_mask, magpo_stream_t stream);
/* The L - 1 aligned training rows of B sampled windows (rec_iql.py:335-350), window b = steps (start[b] + t) % S, t < L, of env env_idx[b]
 * (device i32; env rows are clamped to [0, N), starts taken mod S), in the row order GruActor.seq_fwd reads: (b, t, agent), t < L - 1.
 * o_obs (stride ldo) / o_tot [B][L-1] / o_action / o_reward from steps 0 .. L-2; o_next_obs (stride ldn) / o_next_mask [rows][K] from the same
 * steps' real-next fields; o_next_tot / o_next_terminal [B][L-1] from steps 1 .. L-1.  Only the F leading floats of an output row are written.
 * Rejected: B < 1, L < 2, L > S, NULL indices or outputs, strides < F. */
int magpo_replay_gather(const float* r_obs, const unsigned char* r_mask, const int* r_action, const float* r_reward,
                        const unsigned char* r_terminal, const unsigned char* r_tot, const float* r_next_obs,
                        const unsigned char* r_next_mask, int N, int S, int A, int F, int K, const int* env_idx,
                        const int* start, int B, int L, float* o_obs, long ldo, unsigned char* o_tot, int* o_action,
                        float* o_reward, float* o_next_obs, long ldn, unsigned char* o_next_mask, unsigned char* o_next_tot,
                        unsigned char* o_next_terminal, magpo_stream_t stream);
/* Double-Q TD loss and its backward over R = B (L - 1) A rows (rec_iql.py:366-377, :299-328): next_a = argmax of q_online_next over the
 * legal next actions (first maximum; next_mask [R][K] nullable), target = reward + (1 - next_terminal[r / A]) * gamma * q_target_next[next_a],
 * q_sel = q_online[action].  dq [R][lddq] = 2 (q_sel - target) / R in column action and exactly 0 in every other column up to
 * min(lddq, 64) (what seq_bwd expects of dlogits); loss_out [3] = [q_loss, mean_q, mean_target] by a two-stage reduction in a fixed order
 * (bit-stable), workspace >= 8 * 1024 doubles.  All three Q inputs share the row stride ld.
 * Rejected: R < 1 or not a multiple of A, K > 32, K > ld, K > lddq, lddq not a multiple of 4, any NULL pointer but next_mask. */
int magpo_q_td_loss(const float* q_online, const float* q_online_next, const float* q_target_next, long ld, const int* action,
                    const unsigned char* next_mask, const float* reward, const unsigned char* next_terminal, float gamma,
                    float* dq, long lddq, double* workspace, float* loss_out, long R, int K, int A, magpo_stream_t stream);
/* Target network over the flat parameter vectors.  mode 0: target = tau * online + (1 - tau) * target (optax.incremental_update), two fp32
 * products and one sum, never contracted.  mode 1: target = online when t_train[0] % update_period == 0, else unchanged
 * (optax.periodic_update; t_train a device int, its value before the increment, rec_iql.py:389-396). */
int magpo_target_update(const float* online, float* target, long n, int mode, float tau, const int* t_train,
                        int update_period, magpo_stream_t stream);

/* All L stored steps of B sampled windows (rec_qmix.py:377-395 unrolls over data_full.obs and never reads next_obs), indices as in
 * magpo_replay_gather (clamped env rows, starts mod S): o_obs (stride ldo) / o_mask [rows][K] in row order (b, t, agent), t < L;
 * o_tot [B][L]; o_action [B][L-1][A] from steps 0 .. L-2; o_reward [B][L-1] = agent column 0 of the reward ring of those steps (the team
 * reward, which magpo_team_reward put into every column).  Rejected: B < 1, L < 2, L > S, NULL indices or outputs, ldo < F. */
int magpo_replay_gather_seq(const float* r_obs, const unsigned char* r_mask, const int* r_action, const float* r_reward,
                            const unsigned char* r_terminal, const unsigned char* r_tot, const float* r_next_obs,
                            const unsigned char* r_next_mask, int N, int S, int A, int F, int K, const int* env_idx,
                            const int* start, int B, int L, float* o_obs, long ldo, unsigned char* o_mask, unsigned char* o_tot,
                            int* o_action, float* o_reward, magpo_stream_t stream);
/* jnp.mean(reward, axis=-1) of one env step (rec_qmix.py:287): out [N][A], every agent column = (((r_0 + r_1) + ...) + r_{A-1}) / (float)A in
 * fp32 in that order.  out may be reward itself. */
int magpo_team_reward(const float* reward, float* out, int N, int A, magpo_stream_t stream);

/* ---- QMIX mixing network (csrc/qmix.hip; QMixingNetwork, mava/networks/base.py:276-343; rec_qmix.py:344-425) ----
 * For a row with agent values q[A] and global state s[G]: x = LayerNorm(s) * scale + bias (rstd = rsqrt(max(E[s^2] - E[s]^2, 0) + 1e-6); x = s
 * without norm_env_states); w1 = |Dense(A E)(relu(Dense(64)(x)))|, b1 = Dense(E)(x), hidden = elu(q . w1 + b1); w2 = |Dense(E)(relu(Dense(64)(x)))|,
 * b2 = Dense(1)(relu(Dense(E)(x))); q_tot = hidden . w2 + b2.
 *   dims_host[11] = {A, E, G, F_raw, id_cols, norm_env_states, Tm, Ts, t_off, q mode, K}: E in {32, 64}, 1 <= A, A E <= 512, 1 <= G = A F_raw <= 128.
 *   params + offs_host[16]: ONE parameter buffer and the offsets (floats, multiples of 4) of its entries, Dense kernels [in][out]:
 *     hyper_w1 Dense_0 kernel [G][64], bias | hyper_w1 Dense_1 kernel [64][A E], bias | hyper_b1 Dense_0 kernel [G][E], bias |
 *     hyper_w2 Dense_0 kernel [G][64], bias | hyper_w2 Dense_1 kernel [64][E], bias | hyper_b2 Dense_0 kernel [G][E], bias |
 *     hyper_b2 Dense_1 kernel [E][1], bias [1] | layer_norm scale [G], bias [G].
 *   Mixer row r is step r % Tm of sequence r / Tm; it reads team (r / Tm) Ts + r % Tm + t_off of the observation rows (Tm = Ts, t_off = 0: row
 *   r reads team r).  The state is never materialised: s = the concatenation over the team's agents j of obs[team A + j][id_cols .. id_cols +
 *   F_raw) (row stride ldo), the layout of magpo_global_state.
 *   q mode 0: q [R][A].  Mode 1: q = Q rows [teams A][ldq], K valid columns, and agent a of row r takes column index[r A + a] (clamped to
 *   [0, K)) of row team A + a.  Mode 2 (double-Q selection): the column is the first maximum of q_online's row over the legal actions
 *   (mask [teams A][K] u8, nullable), taken from q's row.  q_used [R][A] (nullable without save) receives the values that were mixed.
 * magpo_qmix_fwd: q_tot [R] in ONE launch.  save (nullable) = the training mode: [R][magpo_qmix_save_floats(E, G)] floats per row, the two
 *   64-wide hypernetwork hiddens | hyper_b2's hidden [E] | hidden [E] | xhat [round4(G)] (s itself without normalisation) | rstd.
 * magpo_qmix_bwd: from dq_tot [R], one launch + magpo_reduce_slabs: dq [R][A] (nullable) and grads [P] = the gradient of every entry at the
 *   offsets of params (padding between entries zero; the layer_norm entries zero without normalisation).  slab: workspace of
 *   magpo_qmix_bwd_grid(R) * P floats, 16-byte aligned; per-workgroup partial sums folded in a fixed order: no atomics, equal inputs give equal
 *   bits.  d|x|/dx = sign(x) with sign(0) = 0; elu' = 1 for x > 0, else exp(x).  dq64 (nullable; needs index, lddq = 64, K): the scatter for
 *   seq_bwd: row team A + a of dq64 takes dq[r][a] in column index[r A + a] and zero in its other 63 columns; rows of teams that no mixer row
 *   reads are not written.  dims / offsets as the forward's (the q mode is not read).
 * Rejected before a pointer is touched: a shape outside the limits above, R < 1, table sizes other than 11 / 16, an offset that is negative,
 *   not a multiple of 4 or (bwd) outside P, strides that do not cover their rows, a NULL pointer in a required slot. */
long magpo_qmix_save_floats(int E, int G);
long magpo_qmix_bwd_grid(long R);
int magpo_qmix_fwd(const int* dims_host, int ndims, const float* params, const long* offs_host, int noffs, const float* obs, long ldo,
                   const float* q, const float* q_online, long ldq, const int* index, const unsigned char* mask, float* q_tot,
                   float* q_used, float* save, long R, magpo_stream_t stream);
int magpo_qmix_bwd(const int* dims_host, int ndims, const float* params, const long* offs_host, int noffs, long P, const float* save,
                   const float* q_used, const float* dq_tot, float* dq, float* dq64, long lddq, const int* index, float* slab,
                   float* grads, long R, magpo_stream_t stream);
/* TD target and loss of rec_qmix (rec_qmix.py:358-367, :413, :423-425) over R = U B (L - 1) rows (b, t) of U stacked groups: next_done =
 * term_or_trunc [U B][L] at step t + 1 (NOT terminal: QMIX cuts the bootstrap at truncation too); target = reward + (1 - next_done) * gamma *
 * next_q_tot, every operation rounded to fp32 in that order; dq_tot = 2 / R * (q_tot - target); loss_out [8] = [q_loss, mean_q, max_q_error,
 * min_q_error, mean_target, mean_reward_t0, mean_next_qval, done]: sums in double in a fixed order, max / min of err^2 per group averaged over the
 * groups (the reference's pmean), done = mean of term_or_trunc over all L steps.  workspace >= 8 U doubles.
 * Rejected: L < 2, U outside 1..1024, R < 1 or not a multiple of U (L - 1), a NULL pointer. */
int magpo_qmix_td_loss(const float* q_tot, const float* next_q_tot, const float* reward, const unsigned char* term_or_trunc, int L,
                       float gamma, float* dq_tot, double* workspace, float* loss_out, long R, int U, magpo_stream_t stream);

/* ---- K10 optimiser: optax clip_by_global_norm + adam(eps=1e-5) (rec_magpo.py:581-589, :412-420) ---- */
int magpo_clip_adam(float* params, const float* grads, float* mu, float* nu, long n, float grad_scale,
                    float max_norm, float lr, float b1, float b2, float eps, float bc1, float bc2,
                    double* workspace, float* gnorm, magpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MAGPO_H */
