// Internal prototypes of the launch functions implemented in the kernel translation units
// (norm.hip, attention.hip, embed.hip, conv.hip, optim.hip, replay_ring.hip, replay.hip, gemm.hip, gemm_reduce.hip); the schedules in encoder.hip, encoder_bf16.hip
// and cnn_api.hip call these.
#pragma once
#include "common.h"

int layernorm_fwd(const float*, const float*, const float*, float*, float*, float*, int, int, float, int, hipStream_t);
int layernorm_bwd_blocks(int T);
int layernorm_bwd(const float*, const float*, const float*, const float*, const float*, const float*, float*, float*, float*,
                  float*, int, int, int, hipStream_t, ReduceGroup* grp = nullptr);
int rmsnorm_fwd(const float*, long long, const float*, float*, int, int, hipStream_t);
int rmsnorm_bwd_blocks(int B);
int rmsnorm_bwd(const float*, const float*, long long, const float*, float*, long long, float*, float*, int, int, hipStream_t);
int colsum_blocks(int T);
int colsum(const float*, long long, float*, float*, int, int, int, hipStream_t);
int attention_fwd(const float*, float*, float*, int, int, int, int, int, hipStream_t, const LayerDrop* drop = nullptr);
int attention_bwd(const float*, const float*, const float*, const float*, float*, int, int, int, int, int, hipStream_t,
                  const LayerDrop* drop = nullptr);
// attention_long.hip: K / V-tiled attention for any N (the encoder takes it for N > 288 under DGVIT_FLAG_LONG_SEQUENCE); the backward
// needs attention_bwd_tiled_scratch(B, N, H) floats of scratch (delta = rowsum(dO o O) of every row)
int attention_fwd_tiled(const float*, float*, float*, int, int, int, int, int, hipStream_t, const LayerDrop* drop = nullptr);
long long attention_bwd_tiled_scratch(int B, int N, int H);
int attention_bwd_tiled(const float*, const float*, const float*, const float*, float*, float*, long long, int, int, int, int, int,
                        hipStream_t, const LayerDrop* drop = nullptr);
// attention_maps.hip: P = exp2(q.k * scale * log2e - lse) of one layer from its qkv buffer and the forward's lse; rows DGVIT_MAPS_GOAL
// (query 0: probs[b * frame_stride + h * N + k]) or DGVIT_MAPS_ALL (probs[b * frame_stride + (h * N + q) * N + k])
int attention_probs(const float* qkv, const float* lse, float* probs, long long frame_stride, int B, int N, int H, int dh, int rows,
                    hipStream_t st);
// last_block.hip: the last block's attention with K and V folded into token 0's query.  u, r (and du, dr): head h of frame
// b at b * fs + h * D; q / o / dout / dq: B rows of I floats at their row strides; wqkv = to_qkv.weight (3I, D); p (B, H, N) or null.
constexpr long long GOAL_POOL_LDS_MAX = 159 * 1024;      // what a goal_pool workgroup may take at all (the operator entry points)
constexpr long long GOAL_POOL_LDS_BUDGET = 80 * 1024;    // ... and inside the encoder: two workgroups per CU (160 KB); C3 needs 54.5 KB
long long goal_pool_lds_bytes(int N, int D, int H);
bool goal_attention_supports(int N, int D, int H, int dh);
int goal_attention_fwd(const float* xn, const float* wqkv, const float* q, long long ldq, float* o, long long ldo, float* u, float* r,
                       long long fs_ur, float* p, int B, int N, int H, int dh, int D, hipStream_t st);
int goal_attention_bwd_data(const float* xn, const float* wqkv, const float* dout, long long lddo, const float* u, long long fs_ur,
                            const float* p, float* du, float* dr, long long fs_d, float* dq, long long lddq, float* dxn, int B, int N, int H,
                            int dh, int D, hipStream_t st);
int goal_attention_wgrad(const float* q, long long ldq, const float* dout, long long lddo, const float* du, long long fs_d, const float* r,
                         long long fs_ur, float* dwkv, int B, int H, int dh, int D, hipStream_t st);
int patchify(const float*, float*, int, int, int, int, int, hipStream_t);
int add_rows(const float*, long long, const float*, long long, float*, long long, long long, int, hipStream_t);
int goal_row(const float*, const float*, float*, int, int, int, hipStream_t);
int dropout_inplace(float*, long long, unsigned long long, const unsigned long long*, float, hipStream_t);
// transformer-internal dropout of a row block (mask sites 1-3, common.h): dst[r] = (res ? res[r] : 0) + m o src[r] / keep over `rows`
// rows of `width` floats; buffer row r is absolute token row r * rs (mask counter), rows at strides lds / ldd / ldr
int drop_rows(const float* src, long long lds, float* dst, long long ldd, const float* res, long long ldr, long long rows, int width, int rs,
              const LayerDrop& drop, hipStream_t stream);
int relu_bwd(const float*, const float*, float*, long long, hipStream_t);
int adam_step(float*, const float*, float*, float*, long long, float, float, float, float, float, long long, const long long*,
              hipStream_t);
int soft_update(float*, const float*, long long, float, hipStream_t);
// gradient-norm clipping on flat buffers (optim.hip)
int grad_sqnorm_partials(const float* g, long long n, double* partials, int accumulate, hipStream_t);
int grad_clip_coef(const double* partials, float max_norm, float* out, hipStream_t);
int adam_step_scaled(float*, const float*, float*, float*, long long, float, float, float, float, float, long long, const long long*,
                     const float* grad_scale_dev, hipStream_t);
int scale_by_device_scalar(float* x, long long n, const float* scale_dev, hipStream_t);
// Adam / AdamW with parameter groups and a device-side lr schedule, one launch per run (optim.hip)
int adam_step_groups(float* p, const float* g, float* m, float* v, long long n, const long long* seg_end4, const unsigned char* seg_group,
                     int nseg, const float* group_hyper, int ngroups, float* lr_out, float beta1, float beta2, float eps, int decoupled,
                     long long step, long long sched_step, const long long* step_dev, int sched_kind, long long warmup_steps,
                     long long total_steps, float final_ratio, const float* grad_scale_dev, hipStream_t);
// the SAC loss head (sac_loss.hip): one launch per loss, alpha from device memory; done, weights, discount, log_alpha, td and
// grads may be null; discount (B values) takes the place of gamma sample by sample
int sac_critic_loss(const float* q1, const float* q2, const float* reward, const float* done, const float* weights, const float* discount,
                    const float* next_q1, const float* next_q2, const float* next_log_pi, const float* log_alpha, float alpha, float gamma,
                    float* target, float* td, float* loss, float* grads, int B, int A, hipStream_t);
int sac_actor_loss(const float* log_pi, const float* q1_pi, const float* q2_pi, const float* log_alpha, float alpha, int with_temperature,
                   float target_entropy, float* losses, float* grads, float* dlog_alpha, int B, int A, hipStream_t);
int sac_scale_grads(const float* src, float* dst, long long n, const float* scale_dev, hipStream_t);
int sac_bc_loss(const float* pred, const float* action, const void* mask, int mask_u8, const float* q1_demo, const float* q2_demo,
                const float* q1_pi, const float* q2_pi, int nll, float* out, float* grads, int B, int A, hipStream_t);
// the CQL(H) penalty of a twin critic over M proposal actions per row (include/dgvit_hip.h: dgvit_sac_cql_penalty)
int sac_cql_penalty(const float* q1_cat, const float* q2_cat, const float* q1_data, const float* q2_data, const float* log_w, const void* mask,
                    int mask_u8, const float* log_weight, float weight, float temperature, float target_gap, int lagrange, float* out,
                    float* grads, float* dlog_weight, int B, int M, int C, hipStream_t);
int im2col(const float*, float*, int, int, int, int, int, int, int, hipStream_t);
int col2im_relu(const float*, const float*, float*, int, int, int, int, int, int, hipStream_t);
// the (B, H, W, C) frame gradient from conv1's column gradient (rows of KP floats, 25 C real taps): no ReLU mask
int col2im_frame(const float* dcols, float* dx, int B, int H, int W, int C, int OH, int OW, int KP, hipStream_t);
int weight_pack(const float*, float*, int, int, int, int, hipStream_t);
int avgpool(const float*, float*, int, int, int, hipStream_t);
int avgpool_bwd_relu(const float*, const float*, float*, int, int, int, hipStream_t);
// replay_ring.hip: the replay ring's storage kernels, fp32 and uint8 frames (formulas: include/dgvit_hip.h)
int gather_rows(const float*, const long long*, float*, long long, long long, long long, hipStream_t);
// gather_rows with the random shift of a (H, W) frame folded in (idx / shifts_out may be null; draw: the shift table in common.h)
int gather_shift_frames(const float* src, const long long* idx, float* out, int* shifts_out, long long nsel, int H, int W,
                        long long row_floats, long long nrows, int pad, int stream_id, unsigned long long seed,
                        const unsigned long long* seed_dev, hipStream_t stream);
int quantize_rows_u8(const float* src, long long src_ld, unsigned char* ring, long long n, long long cols, long long row_bytes,
                     long long nrows, long long start, hipStream_t stream);
int gather_rows_u8(const unsigned char* ring, const long long* idx, float* out, long long nsel, long long cols, long long row_bytes,
                   long long row_floats, long long nrows, hipStream_t stream);
int gather_shift_frames_u8(const unsigned char* ring, const long long* idx, float* out, int* shifts_out, long long nsel, int H, int W,
                           long long row_bytes, long long row_floats, long long nrows, int pad, int stream_id, unsigned long long seed,
                           const unsigned long long* seed_dev, hipStream_t stream);
// episode flags of the ring's slots and the n-step walk along them (include/dgvit_hip.h: n-step returns)
int ring_mark(unsigned char* flags, long long nrows, long long start, long long n, hipStream_t stream);
int nstep_walk(const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags, const float* next_small,
               long long small_ld, const long long* idx, long long nsel, long long nrows, int n, double gamma, float* ret_out, float* done_out,
               float* discount_out, float* next_small_out, int* steps_out, long long* tail_out, hipStream_t stream);
// the ring of E parallel environments: the store path that reads device memory only -- since DESIGN 3.36 the one store path of add and
// add_batch as well -- and the walk with a stride
int ring_store_frames(const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8, long long src1_ld, void* ring0,
                      void* ring1, int ring_u8, long long ring_ld, long long n, long long cols, long long nrows, long long start,
                      hipStream_t stream);
int ring_store_small(const dgvit_small_fields& fields, unsigned char* flags, const void* episode_end, int end_f32, long long n,
                     long long nrows, long long start, hipStream_t stream);
int nstep_walk_strided(const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags,
                       const float* next_small, long long small_ld, const long long* idx, long long nsel, long long nrows, long long stride,
                       int n, double gamma, float* ret_out, float* done_out, float* discount_out, float* next_small_out, int* steps_out,
                       long long* tail_out, hipStream_t stream);
// the ring that stores each frame once: the bookkeeping of a store, its frames into the one arena, and the arena rows of sampled slots'
// next_obs (include/dgvit_hip.h: The ring that stores each frame once)
int ring_plan_next(int* next_row, long long* state, int* moves, const float* done, long long done_ld, const unsigned char* flags, long long n,
                   long long nrows, long long start, long long envs, long long pool, hipStream_t stream);
int ring_store_frames_shared(const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8, long long src1_ld, void* arena,
                             const int* moves, int ring_u8, long long ring_ld, long long n, long long cols, long long nrows, long long start,
                             long long envs, long long pool, hipStream_t stream);
int ring_next_rows(const int* next_row, const long long* idx, long long* out, long long nsel, long long nrows, hipStream_t stream);
// frame stacks at sample time: the backward walk that names each sample's K frame rows, the two gathers that interleave them channel-last,
// and the acting side's stack (include/dgvit_hip.h: Frame stacks)
int ring_stack_rows(const long long* idx, const long long* tail, const unsigned char* flags, const float* done, long long done_ld,
                    const int* next_row, long long* obs_rows, long long* next_rows, long long nsel, long long nrows, long long envs, int frames,
                    int full, long long arena_rows, hipStream_t stream);
int gather_stack_frames(const void* src0, const void* src1, const long long* rows, float* out, long long nsel, long long cols, int frames,
                        int ring_u8, long long ring_ld, long long row_floats, long long nrows0, long long nrows1, hipStream_t stream);
int gather_shift_stack_frames(const void* src0, const void* src1, const long long* rows, float* out, int* shifts_out, long long nsel, int H,
                              int W, int frames, int ring_u8, long long ring_ld, long long row_floats, long long nrows0, long long nrows1,
                              int pad, int stream_id, unsigned long long seed, const unsigned long long* seed_dev, hipStream_t stream);
int frame_stack_push(float* stack, const float* frame, long long frame_ld, const unsigned char* reset, int reset_all, long long envs,
                     long long cols, int frames, hipStream_t stream);
// the ring as a file: ages [a0, a0 + n) of every field packed into one device buffer (include/dgvit_hip.h: The ring as a file)
int ring_export(const dgvit_ring_view& ring, void* out, long long out_bytes, long long cols, long long nrows, long long oldest, long long a0,
                long long n, hipStream_t stream);
int per_set_leaves(float* tree, long long capacity, long long first, long long count, const float* leaves, hipStream_t stream);
// replay.hip: prioritized replay on a radix-64 sum / min tree in one fp32 buffer (layout and draw: include/dgvit_hip.h)
long long per_tree_floats(long long capacity);   // -1 outside [1, 2^24]
int per_init(float* tree, long long capacity, hipStream_t stream);
int per_set_range(float* tree, long long capacity, long long first, long long count, hipStream_t stream);
int per_update(float* tree, long long capacity, long long stored, const long long* idx, const float* prio, long long n, float alpha, float eps,
               hipStream_t stream);
int per_sample(const float* tree, long long capacity, const float* uniforms, long long n, int stratified, float beta, long long* idx_out,
               float* weights_out, hipStream_t stream);
int mean_bwd(const float*, float*, int, int, int, hipStream_t);
int depth_normalize_u8(const float*, float*, float*, int, int, int, hipStream_t);
long long depth_normalize_scratch_floats(int);
int noise_clip(const float*, const float*, float*, long long, float, unsigned long long, hipStream_t);
int gaussian_blur_band(const float*, float*, float*, int, int, int, int, int, int, hipStream_t);
int resize_bilinear(const float*, float*, int, int, int, int, int, float, hipStream_t);
int mlp_head_forward(const dgvit_mlp_desc*, const float* const*, const float* const*, float*, float*, float*, hipStream_t);
long long mlp_head_backward_scratch(const dgvit_mlp_desc*);
int mlp_head_backward(const dgvit_mlp_desc*, const float* const*, const float* const*, const float*, const float*, const float* const*,
                      float* const*, float* const*, float*, long long, hipStream_t);
// the same head with input pieces shared by groups of share[s] consecutive head rows (include/dgvit_hip.h)
int mlp_head_forward_shared(const dgvit_mlp_desc*, const int* share, const float* const*, const float* const*, float*, float*, float*, hipStream_t);
long long mlp_head_backward_shared_scratch(const dgvit_mlp_desc*, const int* share);
int mlp_head_backward_shared(const dgvit_mlp_desc*, const int* share, const float* const*, const float* const*, const float*, const float*,
                             const float* const*, float* const*, float* const*, float*, long long, hipStream_t);
int tanh_gaussian_forward(const float*, const float*, const float*, const float*, const float*, int, float, float, float*, float*, float*,
                          int, int, hipStream_t);
int tanh_gaussian_backward(const float*, const float*, const float*, const float*, int, float, float, const float*, const float*,
                           const float*, float*, float*, int, int, hipStream_t);
// log pi(a | s) of a given action under the same policy and its gradient for mean and log_std_raw
int tanh_gaussian_log_prob(const float* mean, const float* log_std_raw, const float* action, const float* scale, const float* bias, int scale_n,
                           float ls_min, float ls_max, float* log_prob, int B, int A, hipStream_t);
int tanh_gaussian_log_prob_backward(const float* mean, const float* log_std_raw, const float* action, const float* scale, const float* bias,
                                    int scale_n, float ls_min, float ls_max, const float* d_log_prob, float* dmean, float* dlog_std_raw, int B,
                                    int A, hipStream_t);
// block.hip: two launches per transformer block for small batches (no-grad forward), cross-workgroup sums inside the launches
bool block_path_supports(int B, int N, int D, int H, int dh, int M);
long long block_path_slab_floats(int B, int N, int D, int H, int M);
long long block_path_counters(int B, int N);
struct BlockFirst {     // block 0 assembling its own token rows (block.hip)
  const float* goal; const float* pos0; float* xres;
  float keep; unsigned long long seed; const unsigned long long* seed_dev;
};
int block_path_layer(const float* x, const float* ln1, float* xout, float* ln1_out, const float* const* lp, const float* const* next_ln,
                     int token0_only, float* slabs, int* counters, const BlockFirst* first, const float* rms_g, float* feat, int B, int N, int D,
                     int H, int dh, int M, hipStream_t st);
// (frame.hip: diagnostic build only)
bool frame_path_supports(int B, int N, int D, int H, int dh, int M);
long long frame_path_scratch_floats(int B, int N, int D, int H, int M);
int frame_path_forward(const float* x0, const float* const* params, int L, float* scratch, float* feat, int B, int N, int D, int H, int dh,
                       int M, hipStream_t st);
