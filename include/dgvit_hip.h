/* libdgvit_hip.so -- C ABI of the MI355X (gfx950) DGViT encoder hot path.
 *
 * The reference (REGRAGUIahmed/DGViT) has no FFI: its boundary is the Python nn.Module surface of
 *   src/vis_nav/vis_nav/GoalFormer.py        (GoT, Transformer, Attention, FeedForward, PreNorm, RMSNorm)
 *   src/vis_nav/vis_nav/got_sac_network.py   (GoTPolicy, GoTQNetwork, DeterministicGoTPolicy)
 * This header is the lower boundary a Python (ctypes) or C++ host binds instead of the aten ops those
 * modules call.  Each entry point names the reference lines it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to a caller-allocated, contiguous fp32 buffer (row-major);
 *   - nothing allocates, frees or synchronises; all work is enqueued on `stream` (a hipStream_t passed
 *     as void*, 0 = the null stream); callable from any host thread (autograd's backward thread too);
 *   - no mutable global state besides one-time initialisation (a helper stream, per-device kernel attributes): there are no
 *     setter functions; the schedule options (DGVIT_FLAG_*) are fields of dgvit_config (`flags`) and travel with every call.  The A/B and
 *     diagnostic knobs of tools/ exist only in the separately built libdgvit_hip_diag.so (include/dgvit_hip_diag.h);
 *   - return value 0 = success, negative = error; dgvit_last_error() gives the thread-local message;
 *   - sizes are element counts unless a name says bytes.
 */
#ifndef DGVIT_HIP_H
#define DGVIT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define DGVIT_ABI_VERSION 7

/* error codes */
#define DGVIT_OK 0
#define DGVIT_ERR_ARG (-1)
#define DGVIT_ERR_HIP (-2)
#define DGVIT_ERR_ALIGN (-3)
#define DGVIT_ERR_WORKSPACE (-4)

int dgvit_abi_version(void);
/* sizeof(dgvit_config) as this library was compiled: a host binding checks its own struct against it before the first call
 * (a struct one field short makes the library read past its end) */
int dgvit_config_size(void);
const char* dgvit_last_error(void);
/* number of visible HIP devices (<0 on error); does not create a context */
int dgvit_device_count(void);

/* ----------------------------------------------------------------------------------------------
 * Encoder shape = the GoT constructor arguments (GoalFormer.py:124-154).  patch_h/patch_w are honoured
 * (the reference hard-wires 16x20, GoalFormer.py:137-139).  dim_head must be 64 or 32; tokens
 * N = (image_h/patch_h)*(image_w/patch_w) + 1 <= 288, or any N with DGVIT_FLAG_LONG_SEQUENCE (fp32 and bf16 paths).
 * -------------------------------------------------------------------------------------------- */
typedef struct dgvit_config {
  int image_h, image_w;
  int patch_h, patch_w;
  int dim;       /* D */
  int depth;     /* L */
  int heads;     /* H */
  int dim_head;  /* dh, inner width I = H*dh */
  int mlp_dim;   /* M */
  int pool_mean; /* 0: pool='cls' (token 0, what the reference's networks use), 1: pool='mean' (GoalFormer.py:167) */
  int flags;     /* schedule options, DGVIT_FLAG_* below (0 = defaults); a forward and its backward must be given the same value */
} dgvit_config;
/* The output reads only token 0 of the last block (GoalFormer.py:167), so by default that block computes Q, the attention output,
 * to_out and the feed-forward for one row per frame (K / V for all) -- identical results, fewer FLOPs.  This flag runs the dense
 * last block instead (A/B measurements; the bf16 training path is always dense). */
#define DGVIT_FLAG_DENSE_LAST_BLOCK 1
/* dgvit_got_backward runs the weight-gradient GEMMs on one internal helper stream (created on first use, ordered against the
 * caller's stream with events only, so it is capturable) beside the data-gradient chain: +3..5 % frames/s at BASELINE config 3 on
 * MI355X, but concurrent kernels stretch each other's durations, so per-kernel timings (dgvit_profile_*, rocprof) stop being
 * interpretable.  Off: everything stays on the caller's stream. */
#define DGVIT_FLAG_WGRAD_OVERLAP 2
/* Lifts the N <= 288 token limit of the encoder, fp32 and bf16: for N > 288 the attention forward and backward run on K / V-tiled
 * kernels that stream 64-row tiles through LDS (dgvit_attention_forward_tiled, dgvit_attention_forward_bf16_tiled below); N <= 288
 * keeps the fused kernels, bit-identical to the flag being unset.  The fp32 backward scratch (dgvit_got_backward_scratch_floats) grows
 * by B*H*N floats when N > 288 and the flag is set; the bf16 sizes (dgvit_got_bf16_workspace_bytes, _backward_scratch_bytes) follow
 * the same formulas at every N.  With the flag unset every size, result and refusal is unchanged. */
#define DGVIT_FLAG_LONG_SEQUENCE 4

/* Parameter / gradient tables: arrays of DGVIT_NUM_GLOBAL_PARAMS + DGVIT_PARAMS_PER_LAYER*depth device
 * pointers in this order (reference state_dict key in brackets, prefix "trans."):
 *   0 pos_embedding (1,N,D)                         [pos_embedding]
 *   1 patch weight (D, patch_h*patch_w)             [to_patch_embedding.1.weight]
 *   2 patch bias (D)                                [to_patch_embedding.1.bias]
 *   3 final RMSNorm gain (D)                        [layer_norm.g]
 *   then for layer i (prefix transformer.layers.i.):
 *   +0 LN1 weight (D) [0.norm.weight]   +1 LN1 bias (D) [0.norm.bias]
 *   +2 to_qkv weight (3I, D) [0.fn.to_qkv.weight]
 *   +3 to_out weight (D, I) [0.fn.to_out.0.weight]  +4 to_out bias (D) [0.fn.to_out.0.bias]
 *   +5 LN2 weight (D) [1.norm.weight]   +6 LN2 bias (D) [1.norm.bias]
 *   +7 MLP fc1 weight (M, D) [1.fn.net.0.weight]    +8 fc1 bias (M) [1.fn.net.0.bias]
 *   +9 MLP fc2 weight (D, M) [1.fn.net.3.weight]    +10 fc2 bias (D) [1.fn.net.3.bias]
 * cls_token and mlp_head.* never take part in the forward (GoalFormer.py:143,151-154) and are not passed.
 * heads == 1 and dim_head == dim: the reference's Attention has NO output projection (to_out = nn.Identity(), GoalFormer.py:56,66-69);
 * slots +3 / +4 are then ignored in both tables (pass NULL) and the attention output joins the residual stream directly (fp32 path;
 * the bf16 entry points refuse that shape). */
#define DGVIT_NUM_GLOBAL_PARAMS 4
#define DGVIT_PARAMS_PER_LAYER 11

/* floats of activation workspace the forward needs for `batch` frames.
 * save_for_backward != 0: every layer keeps its activations (input of dgvit_got_backward);
 * == 0: layers reuse one set of buffers (inference). */
long long dgvit_got_workspace_floats(const dgvit_config* cfg, int batch, int save_for_backward);
/* floats of scratch dgvit_got_backward needs (gradient temporaries, split-K slabs, reduction partials) */
long long dgvit_got_backward_scratch_floats(const dgvit_config* cfg, int batch);

/* GoT.forward (GoalFormer.py:156-171) incl. Transformer/PreNorm/Attention/FeedForward/RMSNorm
 * (GoalFormer.py:31-122).
 *   img  (B, image_h, image_w)   goal (B, D)   ->   feat (B, D)
 * dropout_keep < 1 applies train-mode nn.Dropout(emb_dropout) (GoalFormer.py:163) with a Philox mask
 * derived from dropout_seed; pass 1.0f for eval mode.  dropout_seed_dev (may be NULL): a DEVICE pointer to the
 * seed, read by the kernel at run time and overriding dropout_seed -- the form to use inside a captured HIP
 * graph, where a by-value seed would be frozen into every replay. */
int dgvit_got_forward(const dgvit_config* cfg, const float* const* params, const float* img, const float* goal,
                      float* feat, float* workspace, long long workspace_floats, int batch, int save_for_backward,
                      float dropout_keep, unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev,
                      void* stream);

/* Gradient of dgvit_got_forward (what autograd derives for GoalFormer.py:156-171).
 *   dfeat (B, D) -> grads[] (same table order as params, each written, not accumulated), dgoal (B, D).
 * A NULL entry of grads[] marks a frozen parameter (requires_grad off, e.g. the heads-only optimiser of DRL.py:145-148 with the
 * encoder frozen): its weight-gradient GEMM / reduction is skipped.
 * `workspace` is the buffer the matching forward (save_for_backward=1) filled; same dropout_keep/seed. */
int dgvit_got_backward(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                       float* dgoal, const float* workspace, long long workspace_floats, float* scratch,
                       long long scratch_floats, int batch, float dropout_keep, unsigned long long dropout_seed,
                       const unsigned long long* dropout_seed_dev, void* stream);

/* Gradient-ready events: the data-parallel gradient exchange (RCCL all-reduce, one bucket per transformer block) can start while the
 * backward is still running on earlier blocks.  dgvit_got_backward_ev / dgvit_got_backward_bf16_ev are dgvit_got_backward /
 * dgvit_got_backward_bf16 with one more argument: events the call RECORDS ON `stream` at the point where a group of parameter
 * gradients is final (all split-K slab sums and LayerNorm partial sums included):
 *   head      after the final-norm gradient (grads[3]), before the last block's backward;
 *   layer[i]  after every gradient of transformer block i (grads[4 + 11 i .. 4 + 11 i + 10]); blocks finish in the order L-1 .. 0.
 * The embedding gradients (grads[0..2]) are final when the call's work on `stream` is.  NULL entries are skipped; events == NULL is
 * the plain call.  Events are hipEvent_t handles: the caller's own, or made by dgvit_event_create (timing disabled).  A consumer on
 * another stream orders itself with dgvit_stream_wait_event (= hipStreamWaitEvent) -- host code never blocks.
 * (The reference has no counterpart: torch DDP's bucket hooks on autograd, which one fused backward call bypasses.) */
typedef struct dgvit_grad_events {
  int n_layers;        /* must equal cfg->depth */
  void* const* layer;  /* [n_layers] hipEvent_t or NULL */
  void* head;          /* hipEvent_t or NULL */
} dgvit_grad_events;
int dgvit_event_create(void** event);
int dgvit_event_destroy(void* event);
int dgvit_stream_wait_event(void* stream, void* event);
int dgvit_got_backward_ev(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                          float* dgoal, const float* workspace, long long workspace_floats, float* scratch,
                          long long scratch_floats, int batch, float dropout_keep, unsigned long long dropout_seed,
                          const unsigned long long* dropout_seed_dev, void* stream, const dgvit_grad_events* events);

/* Transformer-internal dropout (fp32 path): dgvit_got_forward_v2 / dgvit_got_backward_v2 / dgvit_got_backward_v2_ev are the calls
 * above with one more argument, layer_dropout_keep in (0, 1] (= 1 - GoT(dropout=p); 1.0f in eval mode).  The entry points above
 * are these with layer_dropout_keep = 1.  Below 1, train-mode nn.Dropout(dropout) is applied at the four sites of every transformer
 * block (GoalFormer.py:47, 49, 68, 78); emb-dropout (dropout_keep) and these masks share dropout_seed / dropout_seed_dev; nothing is
 * stored -- the backward regenerates every mask, so pass it the forward's keeps and seed.  The mask: Philox4x32-10 keyed by the seed,
 * an element is kept when r * 2^-32 < keep and scaled by 1/keep; emb-dropout uses counter word z = 0, site s of layer l uses
 * z = 0x44000000 | (l << 2) | s, and (x, y) = the 64-bit index i4 of the element's float4 group, lane = index % 4:
 *   s = 0  attention probabilities (b, h, q, k) after softmax  i4 = ((b*H + h)*N + q)*ceil(N/4) + k/4, lane k % 4
 *   s = 1  to_out output (token row, D), before the residual   i4 = (row*D + c)/4
 *   s = 2  FeedForward hidden (token row, mlp_dim), after GELU  i4 = (row*mlp_dim + c)/4
 *   s = 3  FeedForward output (token row, D), before the residual
 * row = b*N + t, the absolute token row.  Projection-less attention (heads == 1, dim_head == dim) has no site 1.  The bf16 entry points
 * that take it are dgvit_got_forward_bf16_v2 and its companions below.  Returns DGVIT_ERR_ARG when layer_dropout_keep is outside (0, 1]. */
int dgvit_got_forward_v2(const dgvit_config* cfg, const float* const* params, const float* img, const float* goal,
                         float* feat, float* workspace, long long workspace_floats, int batch, int save_for_backward,
                         float dropout_keep, float layer_dropout_keep, unsigned long long dropout_seed,
                         const unsigned long long* dropout_seed_dev, void* stream);
int dgvit_got_backward_v2(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                          float* dgoal, const float* workspace, long long workspace_floats, float* scratch,
                          long long scratch_floats, int batch, float dropout_keep, float layer_dropout_keep,
                          unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev, void* stream);
int dgvit_got_backward_v2_ev(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                             float* dgoal, const float* workspace, long long workspace_floats, float* scratch,
                             long long scratch_floats, int batch, float dropout_keep, float layer_dropout_keep,
                             unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev, void* stream,
                             const dgvit_grad_events* events);

/* Gradient with respect to the depth frame: dgvit_got_backward_v3 / dgvit_got_backward_v3_ev are dgvit_got_backward_v2 / _v2_ev with
 * one more argument, dimg (B, image_h, image_w) floats, written (not accumulated); NULL = not wanted (the _v2 entry points are these
 * with NULL).  dimg = unpatchify(dx0[patch rows] . W_pe), dx0 the gradient of the assembled tokens, so it INCLUDES the emb-dropout
 * mask (the same mask and 1/keep as dgvit_got_forward's); the transformer-internal masks act on it through dx0 like on every other
 * gradient.  It does not need the patch weight's or bias's gradient: with grads[1] == grads[2] == NULL (a frozen model; saliency maps)
 * only dimg and whatever else grads[] asks for are formed.  Workspace and scratch sizes are those of the _v2 calls; NULL dimg leaves
 * the launches and every other output exactly as _v2 has them. */
int dgvit_got_backward_v3(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                          float* dgoal, float* dimg, const float* workspace, long long workspace_floats, float* scratch,
                          long long scratch_floats, int batch, float dropout_keep, float layer_dropout_keep,
                          unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev, void* stream);
int dgvit_got_backward_v3_ev(const dgvit_config* cfg, const float* const* params, float* const* grads, const float* dfeat,
                             float* dgoal, float* dimg, const float* workspace, long long workspace_floats, float* scratch,
                             long long scratch_floats, int batch, float dropout_keep, float layer_dropout_keep,
                             unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev, void* stream,
                             const dgvit_grad_events* events);

/* ----------------------------------------------------------------------------------------------
 * Attention maps (GoalFormer.py:77): the softmax probabilities of every layer and head, taken before the attention-dropout site
 *   P = softmax(q k^T * dim_head^-1/2)      (fp32 scores, softmax and output; in the bf16 configuration from the bf16 q / k that the
 *                                            attention kernel reads -- not the bf16-rounded P that feeds P V)
 * rows = DGVIT_MAPS_GOAL: query 0 only (the goal token, the one row the networks use)   maps (B, L, H, N)      [b][l][h][k]
 * rows = DGVIT_MAPS_ALL:  every query row                                                maps (B, L, H, N, N)   [b][l][h][q][k]
 * dgvit_got_forward_maps[_bf16] is the no-grad forward (save_for_backward = 0) with the same arguments otherwise, plus `maps` and
 * `rows`: feat is what dgvit_got_forward_v2 / dgvit_got_forward_bf16 return for the same inputs, keeps and seed.  The call always
 * takes the GEMM schedule (never the small-batch block path: feat then agrees with the block path to the usual 2e-5); under
 * DGVIT_MAPS_ALL it runs the last block dense (as DGVIT_FLAG_DENSE_LAST_BLOCK).  After each layer's attention a maps kernel recomputes
 * P from that layer's qkv buffer and the base-2 log-sum-exp the attention forward writes into the workspace.  Workspace: the no-grad
 * sizes apply (dgvit_got_workspace_floats / dgvit_got_bf16_workspace_bytes with save_for_backward = 0); there is no size query of
 * its own.  No allocation and no host sync: capturable like the forward.  A null `maps` or a bad `rows` returns DGVIT_ERR_ARG, and every
 * refusal of the forward (shape, token limit, bf16 restrictions) applies unchanged.
 * -------------------------------------------------------------------------------------------- */
#define DGVIT_MAPS_GOAL 0
#define DGVIT_MAPS_ALL 1
int dgvit_got_forward_maps(const dgvit_config* cfg, const float* const* params, const float* img, const float* goal, float* feat,
                           float* maps, int rows, float* workspace, long long workspace_floats, int batch, float dropout_keep,
                           float layer_dropout_keep, unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev,
                           void* stream);
/* kernel level: qkv (B, N, 3*H*dh) as the encoder's to_qkv output, lse (B, H, N) the base-2 log-sum-exp of dgvit_attention_forward /
 * dgvit_attention_forward_tiled (rows = DGVIT_MAPS_GOAL reads lse[b][h][0] only)  ->  probs (B, H, N) or (B, H, N, N) fp32.
 * dh 64 or 32. */
int dgvit_attention_probs(const float* qkv, const float* lse, float* probs, int B, int N, int H, int dh, int rows, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Head Linears (got_sac_network.py:111,115-121,226,230-234,429,433-435):  y = act(x W^T + b)
 *   x (M, K), w (N, K), b (N) or NULL, y (M, N); act: 0 = identity, 1 = ReLU.
 * -------------------------------------------------------------------------------------------- */
int dgvit_linear_forward(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int act,
                         void* stream);
long long dgvit_linear_backward_scratch_floats(int M, int N, int K);
/* dy (M,N) is the gradient of y; with act = 1 it is masked by (y > 0) first (y = the forward output).
 * Writes dx (M,K) (NULL to skip), dw (N,K), db (N) (NULL to skip). */
int dgvit_linear_backward(const float* dy, const float* x, const float* w, const float* y, float* dx, float* dw,
                          float* db, float* scratch, long long scratch_floats, int M, int N, int K, int act,
                          void* stream);

/* ----------------------------------------------------------------------------------------------
 * Fused MLP heads (got_sac_network.py:114-121 twin Q, :230-235 policy, :433-435 deterministic policy, CNN twins :157-166, :303-307):
 *     y_j = W3_j relu(W2 relu(W1 cat(x_0 .. x_{nseg-1}) + b1) + b2) + b3_j ,  j < heads3,  for `towers` independent towers
 * one launch forward, one backward (+ one grouped reduction when batch > 32), instead of one GEMM / mask / split-K / reduction
 * launch per Linear.  A policy head = 1 tower, 2 third layers (mean_linear, log_std_linear); a twin-Q head = 2 towers
 * (fc1,fc2,fc3 | fc11,fc21,fc31) over the same concatenated input.  n1, n2: multiples of 32 up to 128; n3 <= 4; sum kx <= 512.
 *   in[s]     : (batch, kx[s]) with row stride ldx[s]          (the torch.cat of the reference is never materialised)
 *   params    : per tower  W1 (n1, K0), b1, W2 (n2, n1), b2, then per third layer W3 (n3, n2), b3
 *   h1, h2    : (towers, batch, n1 / n2) post-ReLU activations, kept for the backward
 *   y         : (towers, heads3, batch, n3)
 *   dy        : towers * heads3 pointers to (batch, n3) gradients of the single outputs; NULL = that output is unused: it
 *               contributes nothing and its third layer gets no gradient (like an nn.Linear outside the autograd graph)
 *   din[s]    : (batch, kx[s]) with dense rows (row stride kx[s]) whatever ldx[s] is, NULL to skip;  dparams: like params, NULL
 *               entries skipped (written, not accumulated)
 * Alignment: every pointer is a float pointer (4 bytes).  W2 and every W3 must be 16-byte aligned (DGVIT_ERR_ARG otherwise); the
 * backward reads h1 and h2 in 16-byte pieces, so they must be 16-byte aligned as well.  W1, the biases, the inputs (base and ldx),
 * dy, din, dparams and the scratch take any 4-byte alignment: a W1 that is 16-byte aligned in every tower with K0 % 4 == 0 is read
 * in 16-byte pieces, one that is 8-byte aligned with an even K0 in 8-byte pairs, any other element by element; a dparams entry that
 * is not 16-byte aligned (or whose size is not a multiple of 4) is summed by the scalar form of the reduction when batch > 32.
 * -------------------------------------------------------------------------------------------- */
typedef struct dgvit_mlp_desc {
  int batch, nseg, kx[3], ldx[3];
  int n1, n2, n3, towers, heads3;
} dgvit_mlp_desc;
int dgvit_mlp_head_forward(const dgvit_mlp_desc* desc, const float* const* in, const float* const* params, float* h1, float* h2,
                           float* y, void* stream);
long long dgvit_mlp_head_backward_scratch_floats(const dgvit_mlp_desc* desc);
int dgvit_mlp_head_backward(const dgvit_mlp_desc* desc, const float* const* in, const float* const* params, const float* h1,
                            const float* h2, const float* const* dy, float* const* din, float* const* dparams, float* scratch,
                            long long scratch_floats, void* stream);

/* Shared input pieces: the same head for batch = B * M head rows of which some input pieces hold only B rows -- Q(s, a_m) for M actions
 * per state (CQL, best-of-N): the encoder features of a state are read in place by its M rows, no M-fold copy is made.
 *   share     : const int[nseg].  share[s] = 1: piece s has `batch` rows, as above.  share[s] = M: piece s has batch / M rows (row stride
 *               ldx[s]) and head row r reads its row r / M -- the layout of repeat_interleave(M, 0).  Every share[s] is 1 or one common M,
 *               1 <= M <= 256, batch % M == 0; every restriction above stays.  DGVIT_ERR_ARG otherwise, before any launch.
 *   forward   : h1, h2, y bit-equal to dgvit_mlp_head_forward on the materialised inputs (the workgroup's LDS image is the same).
 *   backward  : dparams and the din of every share[s] = 1 piece bit-equal to dgvit_mlp_head_backward on the materialised inputs.  The
 *               din of a shared piece is (batch / M, kx[s]), dense:  din[b][k] = ((dx[bM][k] + dx[bM+1][k]) + ...) + dx[bM+M-1][k]  in
 *               fp32 in this order, dx[r] the value the unshared backward returns for head row r (tower 0 + tower 1 for a twin head).
 *               The rows go to scratch and one small kernel sums them: no atomics, the same bits on every call.
 *   scratch   : dgvit_mlp_head_backward_shared_scratch_floats(desc, share) floats (-1 for a bad desc / share): the unshared call's plus
 *               batch * kx[s] (rounded up to 4) per shared piece.
 * A share of all ones IS the unshared call: the same launches, the same bits, the same scratch. */
int dgvit_mlp_head_forward_shared(const dgvit_mlp_desc* desc, const int* share, const float* const* in, const float* const* params, float* h1,
                                  float* h2, float* y, void* stream);
long long dgvit_mlp_head_backward_shared_scratch_floats(const dgvit_mlp_desc* desc, const int* share);
int dgvit_mlp_head_backward_shared(const dgvit_mlp_desc* desc, const int* share, const float* const* in, const float* const* params,
                                   const float* h1, const float* h2, const float* const* dy, float* const* din, float* const* dparams,
                                   float* scratch, long long scratch_floats, void* stream);

/* tanh-Gaussian action sampling of GoTPolicy.sample / GaussianPolicy.sample (got_sac_network.py:238-251, 310-321) in one launch:
 *   ls = clamp(log_std_raw, ls_min, ls_max); x = mean + exp(ls) * eps; y = tanh(x); action = y * scale + bias;
 *   log_prob (B) = sum_a [Normal(mean, exp(ls)).log_prob(x) - log(scale * (1 - y^2) + 1e-6)];  tanh_mean = tanh(mean) * scale + bias.
 * mean, log_std_raw, eps, action, tanh_mean: (B, A); scale, bias: `scale_n` = 1 (scalar) or A values; eps ~ N(0, 1) from the caller.
 * backward: gradients of action / log_prob / tanh_mean (NULL = none) -> dmean, dlog_std_raw (the clamp's mask included). */
int dgvit_tanh_gaussian_forward(const float* mean, const float* log_std_raw, const float* eps, const float* scale, const float* bias,
                                int scale_n, float ls_min, float ls_max, float* action, float* log_prob, float* tanh_mean, int B,
                                int A, void* stream);
int dgvit_tanh_gaussian_backward(const float* mean, const float* log_std_raw, const float* eps, const float* scale, int scale_n,
                                 float ls_min, float ls_max, const float* d_action, const float* d_log_prob, const float* d_tanh_mean,
                                 float* dmean, float* dlog_std_raw, int B, int A, void* stream);

/* log pi(a | s) of a GIVEN action under the same policy -- behaviour cloning by maximum likelihood, AWAC/AWR-style extraction, importance
 * ratios (GoTPolicy.log_prob / GaussianPolicy.log_prob).  The density dgvit_tanh_gaussian_forward reports, at y = (action - bias) / scale
 * in the place of tanh(mean + std eps), one launch each way:
 *   y  = clamp((action - bias) / scale, -(1 - 1e-6), 1 - 1e-6)     a demonstration at or beyond the action bound stays finite
 *   x  = atanh(y) = 0.5 log((1 + y) / (1 - y));   ls = clamp(log_std_raw, ls_min, ls_max);   e = (x - mean) exp(-ls)
 *   log_prob[b] = sum_a [ -e^2 / 2 - ls - log(sqrt(2 pi)) - log(scale * (1 - y^2) + 1e-6) ]
 * computed in double from the fp32 inputs and rounded once where a value is stored.  mean, log_std_raw, action: (B, A); log_prob and
 * d_log_prob: B values; scale, bias: `scale_n` = 1 or A values.  backward: dmean = g e exp(-ls), dlog_std_raw = g (e^2 - 1) where
 * log_std_raw lies in [ls_min, ls_max] (bounds included) and 0 elsewhere, g = d_log_prob[b]; nothing is produced for action, scale or bias.
 * B >= 1, 1 <= A <= 16, B * A < 2^31, ls_min <= ls_max; every pointer non-null and 4-byte aligned, else DGVIT_ERR_ARG before any launch. */
int dgvit_tanh_gaussian_log_prob(const float* mean, const float* log_std_raw, const float* action, const float* scale, const float* bias,
                                 int scale_n, float ls_min, float ls_max, float* log_prob, int B, int A, void* stream);
int dgvit_tanh_gaussian_log_prob_backward(const float* mean, const float* log_std_raw, const float* action, const float* scale,
                                          const float* bias, int scale_n, float ls_min, float ls_max, const float* d_log_prob, float* dmean,
                                          float* dlog_std_raw, int B, int A, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Per-operator entry points (used by the encoder above; exported for operator-level parity tests).
 * -------------------------------------------------------------------------------------------- */
/* generic GEMM C = op(A) op(B) (+ epilogue); layout 0 NT (A MxK, B NxK), 1 NN (A MxK, B KxN), 2 TN (A KxM, B KxN).
 * epilogue 0: C = acc + bias + res;  1: C = acc + bias, C2 = gelu(C);  2: C = acc * gelu'(aux);
 *          3: C = relu(acc + bias);  4: C = aux > 0 ? acc : 0;  6: t = acc + bias, C = gelu'(t), C2 = gelu(t);  7: C = acc * aux;
 *          8: C = gelu(acc + bias).  (5 and 9 are internal forms and are refused.)
 * layout 2 runs split over K with `scratch` slabs (dgvit_gemm_scratch_floats) and then reduces into C. */
long long dgvit_gemm_scratch_floats(int layout, int M, int N, int K);
int dgvit_gemm(int layout, int epilogue, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M,
               int N, int K, const float* bias, const float* res, int ldr, float* C2, int ldc2, const float* aux,
               int ldaux, float* scratch, long long scratch_floats, void* stream);

/* nn.LayerNorm(D), eps 1e-5 (GoalFormer.py:34,37): y, and the per-row mean / rstd saved for backward */
int dgvit_layernorm_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            int rows, int D, void* stream);
long long dgvit_layernorm_backward_scratch_floats(int rows, int D);
/* dx = dres + dLN(dy) (dres may be NULL), dgamma, dbeta */
int dgvit_layernorm_backward(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                             const float* dres, float* dx, float* dgamma, float* dbeta, float* scratch,
                             long long scratch_floats, int rows, int D, void* stream);

/* RMSNorm (GoalFormer.py:120-122) on `rows` vectors x[r*ldx .. +D) */
int dgvit_rmsnorm_forward(const float* x, long long ldx, const float* g, float* y, int rows, int D, void* stream);
long long dgvit_rmsnorm_backward_scratch_floats(int rows, int D);
int dgvit_rmsnorm_backward(const float* dy, const float* x, long long ldx, const float* g, float* dx, long long lddx,
                           float* dg, float* scratch, long long scratch_floats, int rows, int D, void* stream);

/* Attention core (GoalFormer.py:73-81): qkv (B, N, 3*H*dh) -> out (B, N, H*dh); scale dh^-1/2; N <= 288, dh 64 or 32.
 * lse (B, H, N): base-2 log-sum-exp of every scaled score row, written by forward (NULL = not kept) and needed by
 * backward, which recomputes the probabilities from it tile by tile (nothing of size N x N is ever stored). */
int dgvit_attention_forward(const float* qkv, float* out, float* lse, int B, int N, int H, int dh, void* stream);
int dgvit_attention_backward(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                             int B, int N, int H, int dh, void* stream);
/* The same attention core on the K / V-tiled kernels the encoder uses for N > 288 under DGVIT_FLAG_LONG_SEQUENCE, for any N >= 1
 * (dh 64 or 32).  nq = number of leading query rows needed (1..N): forward writes out / lse rows < nq and reads every key; backward
 * writes dq rows < nq only and dk / dv for every row.  The backward is deterministic (no atomics) and needs
 * dgvit_attention_backward_tiled_scratch_floats(B, N, H) floats of scratch. */
int dgvit_attention_forward_tiled(const float* qkv, float* out, float* lse, int B, int N, int H, int dh, int nq, void* stream);
long long dgvit_attention_backward_tiled_scratch_floats(int B, int N, int H);
int dgvit_attention_backward_tiled(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* scratch,
                                   long long scratch_floats, int B, int N, int H, int dh, int nq, void* stream);

/* Goal-token attention without K or V (the encoder's last block, where only token 0's query is needed and to_qkv has no bias): with
 * xn (B, N, D) the normalised tokens, wqkv (3*H*dh, D) = to_qkv.weight and q (B rows of H*dh floats, ldq floats apart) token 0's query,
 *   u[b][h] = W_k,h^T q[b][h]   p[b][h] = softmax_t(dh^-1/2 u[b][h] . xn[b][t])   r[b][h] = sum_t p[b][h][t] xn[b][t]   o[b][h] = W_v,h r[b][h]
 * forward writes u, r (B, H, D), p (B, H, N; NULL = not kept) and o (B rows, ldo apart) = what dgvit_attention_forward gives for query
 * row 0 of qkv = xn wqkv^T.  backward takes dout (B rows, lddo apart) and writes dq (B rows, lddq apart), dxn (B, N, D) -- EVERY row, the
 * gradient through K and V only: the caller adds W_q^T dq on the token-0 rows -- and dwkv (2*H*dh, D) = the gradient of rows H*dh.. of
 * wqkv (overwritten; NULL = not wanted); scratch holds dgvit_goal_attention_scratch_floats(B, H, D) floats.  Sums run in a fixed
 * order (no atomics).  dh 64 or 32, D a multiple of 4 up to 1024, N * D floats within 159 KB of LDS; pointers 16-byte aligned, strides
 * multiples of 4. */
long long dgvit_goal_attention_scratch_floats(int B, int H, int D);
/* 1 when a training forward (save != 0) of the encoder and its backward run the last block this way for `cfg` at `batch` frames
 * (token-0 last block, cls pool, no transformer dropout (lkeep == 1), not the K / V-tiled long-sequence attention, dim_head 32 or 64, a
 * frame's N * dim tokens plus 2 * heads * N floats within 80 KB of LDS), 0 when they keep the K / V GEMMs, negative on a bad
 * configuration.  No-grad forwards and attention-maps calls (maps != 0) never fold: their features stay bit-identical to each other.
 * No buffer size depends on it. */
int dgvit_got_last_block_folds(const dgvit_config* cfg, int batch, float layer_dropout_keep, int maps);
int dgvit_goal_attention_forward(const float* xn, const float* wqkv, const float* q, long long ldq, float* o, long long ldo, float* u, float* r,
                                 float* p, int B, int N, int H, int dh, int D, void* stream);
int dgvit_goal_attention_backward(const float* xn, const float* wqkv, const float* q, long long ldq, const float* dout, long long lddo,
                                  const float* u, const float* r, const float* p, float* dq, long long lddq, float* dxn, float* dwkv,
                                  float* scratch, long long scratch_floats, int B, int N, int H, int dh, int D, void* stream);

/* 'b (h p1) (w p2) -> b (h w) (p1 p2)' (GoalFormer.py:138) */
int dgvit_patchify(const float* img, float* patches, int B, int image_h, int image_w, int patch_h, int patch_w,
                   void* stream);
/* in-place dropout with the encoder's Philox stream (n multiple of 4) */
int dgvit_dropout(float* x, long long n, unsigned long long seed, float keep, void* stream);

/* ----------------------------------------------------------------------------------------------
 * CNN feature stack of the shipped critic QNetwork and of GaussianPolicy
 * (got_sac_network.py:129-133,151-155 / 263-266,292-296):
 *   Conv2d(1,16,5,s2) ReLU Conv2d(16,64,5,s2) ReLU Conv2d(64,256,5,s2) ReLU AdaptiveAvgPool2d(1)
 * img (B, H, W) single channel -> feat (B, 256).  params / grads: conv1.weight (16,1,5,5), conv1.bias,
 * conv2.weight (64,16,5,5), conv2.bias, conv3.weight (256,64,5,5), conv3.bias in the reference's layouts.
 * `ws` keeps the three NHWC activations for backward; scratch holds im2col rows, packed weights, split-K slabs.
 * -------------------------------------------------------------------------------------------- */
long long dgvit_cnn_workspace_floats(int B, int H, int W);
long long dgvit_cnn_forward_scratch_floats(int B, int H, int W);
long long dgvit_cnn_backward_scratch_floats(int B, int H, int W);
int dgvit_cnn_forward(const float* img, const float* const* params, float* feat, float* ws, long long ws_floats,
                      float* scratch, long long scratch_floats, int B, int H, int W, void* stream);
int dgvit_cnn_backward(const float* img, const float* const* params, float* const* grads, const float* dfeat,
                       const float* ws, long long ws_floats, float* scratch, long long scratch_floats, int B, int H, int W,
                       void* stream);
/* ... and the gradient with respect to the frame: dimg (B, H, W) floats, written, or NULL = not wanted (dgvit_cnn_backward is this with
 * NULL and every grads[i] required).  A NULL grads[i] marks a frozen parameter: its weight-gradient work is skipped, so a frozen
 * network with dimg set forms only the frame gradient.  Same scratch as dgvit_cnn_backward. */
int dgvit_cnn_backward_v2(const float* img, const float* const* params, float* const* grads, const float* dfeat, float* dimg,
                          const float* ws, long long ws_floats, float* scratch, long long scratch_floats, int B, int H, int W,
                          void* stream);
/* The same stack on frame stacks: conv1 is Conv2d(C,16,5,s2), 1 <= C <= 16 (anything else: DGVIT_ERR_ARG; the sizing functions
 * return -1).  The stack is CHANNEL-LAST: img and dimg are (B, H, W, C) floats, contiguous, channel C - 1 the newest frame -- what
 * sample(frame_stack=C) returns, and conv1's NHWC input as it stands: the result equals nn.Conv2d(C, 16, 5, stride=2) applied to
 * img.permute(0, 3, 1, 2).  params[0] / grads[0] are (16, C, 5, 5), the reference layout of that Conv2d; the other five slots are
 * unchanged.  The entry points above are these with C = 1 (the same launches, bit for bit).  conv1's column matrix of the backward is
 * M1 x al4(25 C) floats (M1 = B * OH1 * OW1; 28 per row for C = 1) and is not chunked: size the scratch with the _v2 functions. */
long long dgvit_cnn_workspace_floats_v2(int B, int H, int W, int C);
long long dgvit_cnn_forward_scratch_floats_v2(int B, int H, int W, int C);
long long dgvit_cnn_backward_scratch_floats_v2(int B, int H, int W, int C);
int dgvit_cnn_forward_v2(const float* img, const float* const* params, float* feat, float* ws, long long ws_floats,
                         float* scratch, long long scratch_floats, int B, int H, int W, int C, void* stream);
int dgvit_cnn_backward_v3(const float* img, const float* const* params, float* const* grads, const float* dfeat, float* dimg,
                          const float* ws, long long ws_floats, float* scratch, long long scratch_floats, int B, int H, int W, int C,
                          void* stream);

/* ----------------------------------------------------------------------------------------------
 * the step BEFORE the path.  The reference samples numpy batches from cpprb and copies
 * (B,128,160) fp32 obs / next_obs to the device every step (DRL.py:375-386).  With the transitions resident in HBM
 * (dgvit_amd.replay.DeviceReplayBuffer) a sample is an index draw plus this gather:
 *   out[i][0..row_floats) = src[idx[i]][0..row_floats)      idx: int64 device array, row_floats % 4 == 0
 * -------------------------------------------------------------------------------------------- */
int dgvit_gather_rows(const float* src, const long long* idx, float* out, long long nsel, long long row_floats,
                      long long nrows, void* stream);

/* The same gather with the DrQ random shift of a (H, W) frame folded into the pass (no extra traffic):
 *   out[i][y][x] = src[clamp(idx[i], 0, nrows-1)][clamp(y + dy_i, 0, H-1)][clamp(x + dx_i, 0, W-1)]
 * which is F.pad(frame, pad, mode="replicate") cropped at offset (pad + dy_i, pad + dx_i); dy_i, dx_i in [-pad, pad].
 * Rows of src and out are row_floats long (a multiple of 4, >= H*W, <= 2^25); columns H*W .. row_floats of out are written as zeros, so
 * pad == 0 gives the bytes of dgvit_gather_rows whenever those columns of src are zero (DeviceReplayBuffer keeps them zero).
 * idx == NULL: the identity (src row i, i clamped to nrows-1).  shifts_out (int32, nsel x 2: dy then dx) is written when non-NULL.
 * Draw: Philox4x32-10 keyed by the seed (seed_dev, when non-NULL, is a device pointer read at run time: graph capture), counter
 * (i, 0, 0x53000000 | stream_id, 0); output word 0 gives dy and word 1 gives dx as (int)(((uint64)r * (2*pad+1)) >> 32) - pad.
 * stream_id in [0, 65536) separates draws that share a seed (DeviceReplayBuffer: 0 = obs, 1 = next_obs).
 * 0 <= pad < min(H, W); 1 <= nsel < 2^24; src and out 16-byte aligned. */
int dgvit_gather_shift_frames(const float* src, const long long* idx /* may be NULL */, float* out, int* shifts_out /* may be NULL */,
                              long long nsel, int H, int W, long long row_floats, long long nrows, int pad, int stream_id,
                              unsigned long long seed, const unsigned long long* seed_dev, void* stream);

/* ----------------------------------------------------------------------------------------------
 * The replay ring with uint8 frame storage (dgvit_amd.replay.DeviceReplayBuffer(frame_dtype=torch.uint8)).  The reference's
 * frames are k / 255 with k in 0..255 (env_lab.py:420-434), so a ring row is row_bytes = al16(H*W) BYTES, a quarter of the fp32 ring, and
 * the fp32 frame is restored inside the gather.  Stored value = code / 255; inputs outside [0, 1] clamp; exact for k / 255 frames and
 * round-to-nearest (half to even) otherwise.  The three calls share these rules: row_bytes % 16 == 0 and row_bytes >= cols; an output row
 * is row_floats floats, a multiple of 4 and >= cols; ring and out 16-byte aligned; columns at or beyond cols of every row WRITTEN (ring
 * rows by the quantiser, output rows by the gathers) are zeros; all index arithmetic is 64-bit.
 *
 * dgvit_quantize_rows_u8:  ring[(start + i) % nrows][c] = q(src[i * src_ld + c])   for i < n, c < cols
 *     q(x) = (uint8) rintf(fminf(fmaxf(x * 255.0f, 0), 255))      half to even; NaN, -0 and -inf store 0, +inf stores 255
 *   The ring wrap happens inside the one launch.  src_ld >= cols is in floats (src 4-byte aligned), so src may be a column block of a
 *   staged matrix or a frame tensor.  0 <= start < nrows, 1 <= n <= nrows, cols <= 2^25.  No longer used by the Python
 *   package, whose one store path is dgvit_ring_store_frames + dgvit_ring_store_small.
 * dgvit_gather_rows_u8:    out[i][c] = (float)ring[clamp(idx[i], 0, nrows-1)][c] / 255.0f      for i < nsel, c < cols
 *   The correctly rounded quotient, bit-equal to numpy's and CPU torch's uint8 -> float32 / 255.  A multiplication by 1.0f / 255.0f is
 *   not (it differs in 126 of the 256 codes); the kernels form the quotient as that product plus one Newton correction in two fused
 *   multiply-adds, equal to the division on every code.
 * dgvit_gather_shift_frames_u8:  dgvit_gather_shift_frames over a byte ring, cols = H * W:
 *     out[i][y][x] = (float)ring[clamp(idx[i], 0, nrows-1)][clamp(y + dy_i, 0, H-1) * W + clamp(x + dx_i, 0, W-1)] / 255.0f
 *   with the same Philox draw and tag, stream_id, seed / seed_dev, shifts_out, idx == NULL identity and clamping, so one seed gives the same
 *   shift table as the fp32 call.  pad == 0 gives the bytes of dgvit_gather_rows_u8.  0 <= pad < min(H, W); 1 <= nsel < 2^24;
 *   row_floats <= 2^25.
 * -------------------------------------------------------------------------------------------- */
int dgvit_quantize_rows_u8(const float* src, long long src_ld, unsigned char* ring, long long n, long long cols, long long row_bytes,
                           long long nrows, long long start, void* stream);
int dgvit_gather_rows_u8(const unsigned char* ring, const long long* idx, float* out, long long nsel, long long cols, long long row_bytes,
                         long long row_floats, long long nrows, void* stream);
int dgvit_gather_shift_frames_u8(const unsigned char* ring, const long long* idx /* may be NULL */, float* out,
                                 int* shifts_out /* may be NULL */, long long nsel, int H, int W, long long row_bytes, long long row_floats,
                                 long long nrows, int pad, int stream_id, unsigned long long seed, const unsigned long long* seed_dev,
                                 void* stream);

/* ----------------------------------------------------------------------------------------------
 * n-step returns at sample time (dgvit_amd.replay: sample(..., n_step=, gamma=)).  Consecutive ring slots are consecutive
 * environment steps, so the multi-step target of cpprb's Nstep option is a walk along the ring.  What the walk may not cross is kept in
 * one byte per slot, `flags` (nrows bytes on the device):
 *   bit 0, END  (1): the slot's transition is the last of its episode, whatever its `done` says (time limits, truncations)
 *   bit 1, HEAD (2): the slot is the newest one written; its ring successor is the oldest slot or an unwritten one
 *
 * dgvit_ring_mark:  after a store of n slots at `start`:  flags[(start + j) % nrows] = (j == n - 1 ? HEAD : 0)  for j < n, and the slot
 *   before `start` loses HEAD and keeps END unless it was itself just written (n == nrows).  An overwritten slot forgets its marks; exactly
 *   one slot carries HEAD.  One launch.  0 <= start < nrows, 1 <= n <= nrows.
 * dgvit_nstep_walk: for each b < nsel, one wave:
 *     i    = clamp(idx[b], 0, nrows-1),  s_k = (i + k) mod nrows
 *     m    = the number of slots visited: the walk stops behind the first k with done[s_k] != 0 or flags[s_k] != 0, or after n slots
 *     ret_out[b]      = (float) sum_{k<m} gamma^k rew[s_k]      summed in DOUBLE in ascending k, gamma^k the left-to-right product of k
 *                                                               factors in double, rounded to fp32 once
 *     discount_out[b] = (float) gamma^m
 *     done_out[b]     = done[s_{m-1}],   tail_out[b] = s_{m-1} (int64),   steps_out[b] = m (int32)
 *     next_small_out[b][:] = next_small[tail_out[b]][:]         rows of small_ld floats, a multiple of 4, copied as float4
 *   rew and done are read at rew[s * rew_ld] and done[s * done_ld] (the first column of a (nrows, ld) matrix).  1 <= n <= 64,
 *   0 <= gamma <= 1 (a double), 1 <= nsel < 2^31, small_ld <= 2^20; next_small and next_small_out 16-byte aligned.  Every slot index is
 *   taken mod nrows, so no index can fault; no atomics: the result depends on the ring and idx[b] alone, not on b or nsel.  tail_out is an
 *   index tensor for the frame gathers above (next_obs of the n-step transition).  Both calls are capturable and neither synchronises.
 * -------------------------------------------------------------------------------------------- */
#define DGVIT_RING_END 1
#define DGVIT_RING_HEAD 2
int dgvit_ring_mark(unsigned char* flags, long long nrows, long long start, long long n, void* stream);
int dgvit_nstep_walk(const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags,
                     const float* next_small, long long small_ld, const long long* idx, long long nsel, long long nrows, int n, double gamma,
                     float* ret_out, float* done_out, float* discount_out, float* next_small_out, int* steps_out, long long* tail_out,
                     void* stream);

/* ----------------------------------------------------------------------------------------------
 * The ring of E parallel environments (dgvit_amd.replay: DeviceReplayBuffer(num_envs=E), add_vec).  Vector step t lies in
 * the E consecutive slots base .. base + E - 1, base a multiple of E, environment e in slot base + e; E divides nrows, so the successor
 * of slot s in its episode is (s + E) mod nrows and the lane s mod E survives the wrap.  The store path below reads device memory only:
 * a source is a device tensor where it lies, or a column block of one staged matrix.
 *
 * dgvit_ring_store_frames: both frame fields of n consecutive slots in ONE launch; field f in {0, 1} is one grid dimension with its own
 *   source src[f] (element type src_u8[f]: 0 fp32, 1 uint8; row stride src_ld[f] >= cols in ELEMENTS, which need not be a multiple of 4)
 *   and its own ring matrix ring[f] (element type ring_u8, the same for both; row stride ring_ld in elements):
 *     fp32 -> fp32 ring:   ring[(start + i) % nrows][c] = src[i][c]                 ring_ld a multiple of 4 floats
 *     fp32 -> uint8 ring:  ring[(start + i) % nrows][c] = q(src[i][c])              q of dgvit_quantize_rows_u8; ring_ld a multiple of 16
 *     uint8 -> uint8 ring: ring[(start + i) % nrows][c] = src[i][c]                 copied a dword at a time
 *   for i < n, c < cols; columns cols .. ring_ld - 1 of every written row are zeros.  uint8 into an fp32 ring is refused.  A source
 *   whose rows are 16-byte (fp32) or 4-byte (uint8) aligned is read in whole groups, any other element by element: the same bytes.
 *   ring[f] 16-byte aligned, an fp32 source 4-byte aligned; 1 <= n <= nrows, 0 <= start < nrows, cols <= 2^25, ring_ld <= 2^26.
 * dgvit_ring_store_small: the five small fields (dgvit_small_fields: pobs, act, rew, next_pobs, done in any order) of the same n slots
 *   and, when `flags` is not NULL, their marks, in ONE launch:
 *     ring[f][(start + i) % nrows][c] = src[f][i * src_ld[f] + c]   for c < cols[f], zeros up to ring_ld[f] (a multiple of 4 floats)
 *     flags[(start + i) % nrows]      = HEAD | (episode_end && episode_end[i] != 0 ? END : 0)
 *     flags[(start - n + i) % nrows] &= END                         the previous step is no longer the newest; skipped when n == nrows
 *   episode_end may be NULL (no ends); it is n bytes (bool / uint8; end_f32 == 0) or n floats (end_f32 == 1), nonzero = end.  With
 *   flags, n must divide nrows (so the previous step's slots are not the written ones); with flags == NULL nothing but the n written
 *   rows is touched, any 1 <= n <= nrows is taken and the rows may cross the ring's end (add_batch, which marks with dgvit_ring_mark).
 *   1 <= cols[f] <= ring_ld[f] <= 2^20, src_ld[f] >= cols[f].
 * dgvit_nstep_walk_strided: dgvit_nstep_walk with s_k = (i + k * stride) mod nrows, 1 <= stride <= nrows; everything else, every
 *   output and every check as there.  stride == 1 gives the bits of dgvit_nstep_walk.  i + 63 * stride may exceed 2 * nrows (a ring of
 *   fewer than 64 steps): the slot is then reduced by a true modulo, by one subtraction where that is enough.
 * None of the three synchronises; all are capturable.
 * -------------------------------------------------------------------------------------------- */
#define DGVIT_SMALL_FIELDS 5
typedef struct {
  const float* src[DGVIT_SMALL_FIELDS];    /* device rows of field f, src_ld[f] floats apart */
  float* ring[DGVIT_SMALL_FIELDS];         /* (nrows, ring_ld[f]) fp32, 16-byte aligned */
  long long src_ld[DGVIT_SMALL_FIELDS];
  int cols[DGVIT_SMALL_FIELDS];
  int ring_ld[DGVIT_SMALL_FIELDS];
} dgvit_small_fields;
int dgvit_ring_store_frames(const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8, long long src1_ld, void* ring0,
                            void* ring1, int ring_u8, long long ring_ld, long long n, long long cols, long long nrows, long long start,
                            void* stream);
int dgvit_ring_store_small(dgvit_small_fields fields, unsigned char* flags /* may be NULL */, const void* episode_end /* may be NULL */,
                           int end_f32, long long n, long long nrows, long long start, void* stream);
int dgvit_nstep_walk_strided(const float* rew, long long rew_ld, const float* done, long long done_ld, const unsigned char* flags,
                             const float* next_small, long long small_ld, const long long* idx, long long nsel, long long nrows,
                             long long stride, int n, double gamma, float* ret_out, float* done_out, float* discount_out,
                             float* next_small_out, int* steps_out, long long* tail_out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * The ring that stores each frame once (dgvit_amd.replay: DeviceReplayBuffer(shared_next_obs=True)).  Inside an episode
 * the obs of a lane's step t + 1 is the next_obs of its step t, so ONE frame arena of nrows + envs + pool rows (ring format: fp32 rows
 * of ring_ld floats or uint8 rows of ring_ld bytes) replaces the two frame matrices:
 *   rows [0, nrows)                         the obs ring
 *   rows [nrows, nrows + envs)              one pending row per lane: the next_obs of the lane's newest transition
 *   rows [nrows + envs, nrows + envs + pool) the terminal pool, a FIFO: the next_obs of transitions that ended an episode
 * next_row (nrows int32; -1 = never written) names the arena row of every slot's next_obs; state is three int64 {head, tail, lost},
 * counters that only grow: pool entries tail - head are live, entry k lies in pool row k % pool.  Both start as -1s and zeros.
 *
 * dgvit_ring_plan_next: the bookkeeping of a store of n slots at `start`, after dgvit_ring_store_small (and dgvit_ring_mark) of the
 *   same slots, so that done (read at done[s * done_ld]) and flags of a predecessor are the ring's.  For j = 0 .. n - 1 in this order,
 *   s = (start + j) % nrows, p = (s - envs) mod nrows:
 *     1. next_row[s] inside the pool: ++head (the overwritten slot's entry is free)
 *     2. next_row[s] = nrows + s % envs, the lane's pending row
 *     3. p counts when nrows > envs, next_row[p] != -1 and p is not one of the call's own later rows (n == nrows, j < envs: that
 *        transition is already overwritten); it is terminal when done[p] != 0 or flags[p] has END
 *     4. p not terminal:                 next_row[p] = s                       moves[j] = -1
 *     5. p terminal, tail - head < pool: next_row[p] = nrows + envs + tail % pool = moves[j], ++tail
 *     6. p terminal, the pool full:      next_row[p] = p, ++lost                moves[j] = -1   (the slot's own obs stands in)
 *   moves (n int32) tells dgvit_ring_store_frames_shared which rows carry a frame into the pool.  One launch of one wave, 64 rows a
 *   round: the loads and stores of a round are parallel, the FIFO's counters are advanced in row order; no atomics; deterministic.
 *   envs divides nrows, n and start; 1 <= pool <= nrows; nrows + envs + pool < 2^31.
 * dgvit_ring_store_frames_shared: the frames of the same store in ONE launch, sources and conversions as dgvit_ring_store_frames:
 *     arena[(start + i) % nrows]  = src0[i]                                        the obs rows
 *     arena[moves[j]]             = j < envs ? arena[nrows + j] : src1[j - envs]   where moves[j] is a pool row: the terminal
 *                                                                                  predecessor's next_obs, out of the pending row or
 *                                                                                  out of the call's own rows
 *     arena[nrows + l]            = src1[last row of lane l in the call]           l < envs, after the move out of that row
 *   A move out of a pending row and the write over it are one thread's per pixel group, in that order.
 * dgvit_ring_next_rows: out[i] (int64) = next_row[clamp(idx[i], 0, nrows-1)], the index tensor of the next_obs gather over the arena
 *   (dgvit_gather_rows[_u8], dgvit_gather_shift_frames[_u8] with nrows = the arena's rows); a slot never written gives itself.
 * None of the three synchronises; all are capturable.
 * -------------------------------------------------------------------------------------------- */
int dgvit_ring_plan_next(int* next_row, long long* state, int* moves, const float* done, long long done_ld, const unsigned char* flags,
                         long long n, long long nrows, long long start, long long envs, long long pool, void* stream);
int dgvit_ring_store_frames_shared(const void* src0, int src0_u8, long long src0_ld, const void* src1, int src1_u8, long long src1_ld,
                                   void* arena, const int* moves, int ring_u8, long long ring_ld, long long n, long long cols,
                                   long long nrows, long long start, long long envs, long long pool, void* stream);
int dgvit_ring_next_rows(const int* next_row, const long long* idx, long long* out, long long nsel, long long nrows, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Frame stacks (dgvit_amd.replay: sample(..., frame_stack=K), FrameStack).  The ring keeps single frames; the stack of the
 * K newest frames of a slot's episode, channel-last (H, W, K) with channel K - 1 the newest, exists only at sample time.  The n-step
 * walk goes forward along an episode; this is the same walk backward.  1 <= frames = K <= 16.
 *
 * dgvit_ring_stack_rows: for each b < nsel, one wave.  s = clamp(idx[b], 0, nrows-1), E = envs, pred_0 = s, pred_k = (s - k E) mod nrows.
 *   Predecessor k >= 1 is LINKED iff k E < nrows, and s - k E >= 0 or full != 0 (the caller's "every slot is written", by value), and
 *   flags[pred_k] == 0 and done[pred_k * done_ld] == 0 -- where the n-step walk stops, seen from the slot behind.  d = the number of
 *   consecutive linked predecessors from k = 1.  Then (int64, K per sample)
 *     obs_rows[b][c]  = pred_min(K-1-c, d)                             c < K: frames from before the episode's first slot repeat it
 *     next_rows[b][c] = pred^t_min(K-2-c, d_t)                         c < K - 1, rows of the OBS matrix
 *     next_rows[b][K-1] = next_row ? next_row[t] (t where that is no arena row) : t      a row of the NEXT_OBS matrix / the arena
 *   with t = clamp(tail[b]) and d_t walked back from t when tail is not NULL (an n-step sample: dgvit_nstep_walk's tail_out), else
 *   t = s and d_t = d.  envs divides nrows; arena_rows is the arena's row count with next_row and nrows without.  Every row is a slot
 *   of the ring or a row of the arena; no atomics.
 * dgvit_gather_stack_frames: out[b][p * K + c] = fp32(src_c[clamp(rows[b][c])][p]) for p < cols, c < K, zeros up to row_floats, a
 *   multiple of 4 and at least cols * K: the (B, H, W, K) batch.  src_c = src1 for c == K - 1 and src0 before (rows clamped to nrows1 and
 *   nrows0): obs passes its matrix twice, next_obs the obs matrix and its own -- or the arena twice.  ring_u8: 0 fp32 rows of ring_ld
 *   floats (a multiple of 4), 1 byte rows of ring_ld bytes (a multiple of 16), returned as code / 255 like dgvit_gather_rows_u8.  One
 *   launch: a thread reads one float4 / one dword (4 pixels) of each of the K frames and forms the 4 K contiguous floats as K float4s,
 *   which a workgroup stores in output order, 4 KiB per store, through 4 K KiB of LDS.  row_floats may exceed al4(cols * K): every
 *   float up to row_floats is written, zeros behind the stack.
 *   cols * K <= 2^27, 1 <= nsel < 2^24; src0, src1, out 16-byte aligned.
 * dgvit_gather_shift_stack_frames: the same with the random shift of dgvit_gather_shift_frames, ONE (dy, dx) per sample for all K channels:
 *     out[b][(y W + x) K + c] = fp32(src_c[rows[b][c]][clamp(y + dy_b, 0, H-1) * W + clamp(x + dx_b, 0, W-1)])
 *   The draw is that call's -- sample index b, stream_id, seed / seed_dev -- so equal seeds give the shift table of the unstacked call;
 *   shifts_out may be NULL.  0 <= pad < min(H, W).
 * dgvit_frame_stack_push: the acting side.  stack is (envs, cols, K) fp32 in place; per environment e and pixel p
 *     stack[e][p][c] = stack[e][p][c + 1] for c < K - 1,  stack[e][p][K - 1] = frame[e * frame_ld + p]
 *   or, where reset_all != 0 or reset[e] != 0 (reset: envs bytes, may be NULL), all K channels = the new frame.  One launch, thread =
 *   pixel.
 * None of the four synchronises; all are capturable.
 * -------------------------------------------------------------------------------------------- */
int dgvit_ring_stack_rows(const long long* idx, const long long* tail /* may be NULL */, const unsigned char* flags, const float* done,
                          long long done_ld, const int* next_row /* may be NULL */, long long* obs_rows, long long* next_rows,
                          long long nsel, long long nrows, long long envs, int frames, int full, long long arena_rows, void* stream);
int dgvit_gather_stack_frames(const void* src0, const void* src1, const long long* rows, float* out, long long nsel, long long cols,
                              int frames, int ring_u8, long long ring_ld, long long row_floats, long long nrows0, long long nrows1,
                              void* stream);
int dgvit_gather_shift_stack_frames(const void* src0, const void* src1, const long long* rows, float* out, int* shifts_out /* may be NULL */,
                                    long long nsel, int H, int W, int frames, int ring_u8, long long ring_ld, long long row_floats,
                                    long long nrows0, long long nrows1, int pad, int stream_id, unsigned long long seed,
                                    const unsigned long long* seed_dev, void* stream);
int dgvit_frame_stack_push(float* stack, const float* frame, long long frame_ld, const unsigned char* reset /* may be NULL */, int reset_all,
                           long long envs, long long cols, int frames, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Prioritized replay (proportional PER, Schaul et al. 2016) on the device: the index draw in front of the gathers, the importance
 * weights and the priority write-back, none of which touches the host (dgvit_amd.replay.PrioritizedDeviceReplayBuffer).
 *
 * One caller-allocated fp32 buffer `tree` of dgvit_per_tree_floats(capacity) floats, 16-byte aligned, holds a radix-64 tree over the
 * ring's `capacity` slots (1 .. 2^24) with a sum and a min for every node:
 *   [0, 64)   header: word 0 = the running max leaf (1.0 after init, as cpprb), word 1 = its value when the last update began,
 *             the rest reserved
 *   level l = 0 .. L-1, one after the other: pad64(n_l) sums, then pad64(n_l) mins;  n_0 = capacity, n_l = ceil(n_{l-1} / 64), and
 *             the last level is the first with n_l <= 64 (the top block; there is no separate root)
 *   floats    = 64 + 2 * sum_l pad64(n_l)      (capacity 64: 192, 65: 448, 4096: 8384, 4097: 8768, 2^24: 34087104)
 * Padding entries and slots never written hold sum 0 and min +inf.  A leaf is clamp((|priority| + eps)^alpha, 2^-64, 2^64).
 * A parent is always recomputed from its 64 children in one fixed order, never updated by a delta: its bits are a function of its
 * children alone, rebuilding twice is harmless, rounding does not accumulate over updates, and no float atomic is used.
 *
 * dgvit_per_tree_floats: host only; -1 when capacity is outside [1, 2^24].
 * dgvit_per_init:       sums 0, mins +inf, max leaf 1.
 * dgvit_per_set_range:  leaves [first, first + count) (inside the ring, count >= 1) take the current max leaf -- what a newly stored
 *                       transition gets -- and their ancestors are rebuilt.
 * dgvit_per_update:     leaf[idx[j]] from prio[j], j < n, 1 <= n < 2^24 (idx int64, prio fp32, both read when the kernels run).
 *                       An index outside [0, stored) is ignored, not clamped.  The sign of a priority is ignored; a non-finite one
 *                       takes the max leaf as it stood when the call began.  alpha == 1 takes no powf: the leaf is |p| + eps, clamped.
 *                       An index that occurs more than once keeps the LARGEST of its new leaves, whatever its old one was (pass 1
 *                       zeroes the addressed leaves, pass 2 is an integer max on the float bits).  The max leaf is raised the same way
 *                       and never falls.  Then one wave per index and level rebuilds the ancestors.  0 <= alpha <= 1, eps >= 0.
 * dgvit_per_sample:     idx_out[j] (int64) and weights_out[j] (fp32) from uniforms[j] in [0, 1] (clamped; read when the kernel runs),
 *                       1 <= n < 2^24, one wave per sample.  total = the sum of the top block;
 *                         mass = u_j * total                                  (stratified == 0)
 *                         mass = ((float)j + u_j) / (float)n * total          (stratified == 1)
 *                       At each level, from the top block down, lane c holds the sum of child c and the wave an inclusive prefix
 *                       (Hillis-Steele, 6 steps); the chosen child is the first with child > 0 and prefix > mass, or, when none
 *                       qualifies (u == 1, or rounding between a parent and the prefix of its children), the last child with a
 *                       nonzero sum; mass <- max(mass - prefix of the children before it, 0) and the wave descends.  A slot with
 *                       leaf 0 or an index >= capacity is never returned; an all-zero tree gives index 0 and weight 1.
 *                         weights_out[j] = (p_min / leaf)^beta,  p_min = the min of the top block,  0 <= beta <= 1 (0: exactly 1)
 *                       which is cpprb's (N P(i))^-beta / max_k w_k: N and total cancel.
 * Every call is capturable in a HIP graph and none synchronises.
 * -------------------------------------------------------------------------------------------- */
long long dgvit_per_tree_floats(long long capacity);
int dgvit_per_init(float* tree, long long capacity, void* stream);
int dgvit_per_set_range(float* tree, long long capacity, long long first, long long count, void* stream);
int dgvit_per_update(float* tree, long long capacity, long long stored, const long long* idx, const float* prio, long long n, float alpha,
                     float eps, void* stream);
int dgvit_per_sample(const float* tree, long long capacity, const float* uniforms, long long n, int stratified, float beta,
                     long long* idx_out, float* weights_out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * The ring as a file (dgvit_amd.replay: save_transitions, load_transitions).  Transitions are numbered by AGE: age a lies
 * in slot (oldest + a) % nrows, oldest = the next slot to be written when the ring is full and 0 before.
 *
 * dgvit_ring_export: the store path's mirror.  Ages [a0, a0 + n) of every field in ONE launch into ONE device buffer `out`, the chunk
 *   that then leaves in one device -> host copy.  The buffer is field-major; block b starts at a multiple of 16 bytes:
 *     obs, next_obs          n dense rows of cols elements in the ring's own format (frame_u8: bytes, else the fp32 bits): the row
 *                            padding of the ring (frame_ld - cols) is not written, nothing is converted
 *     small[0 .. 4]          n rows of small_cols[f] floats (pobs, act, rew, next_pobs, done for the package)
 *     end                    n bytes: flags[slot] & DGVIT_RING_END, zeros when flags is NULL (HEAD is not exported: it is derived)
 *     leaves                 n floats leaves[slot], only when leaves is not NULL (the tree's level-0 sums, tree + 64)
 *   off_0 = 0, off_{b+1} = align16(off_b + bytes_b); out_bytes must cover the last block.  next_obs of a two-matrix ring
 *   (next_row == NULL, next_rows == nrows) is row `slot` of its matrix; of a shared ring (obs = next_obs = the arena, next_rows the
 *   arena's rows) it is arena row next_row[slot], or the slot's own obs row where the table names no arena row -- what
 *   dgvit_ring_next_rows resolves.  A dense frame row is copied 16 bytes at a time when cols * itemsize is a multiple of 16, 4 bytes at
 *   a time when it is a multiple of 4, else by bytes; every offset is 64-bit.  obs, next_obs and out 16-byte aligned, frame_ld a
 *   multiple of 4 floats / 16 bytes, 1 <= n, 0 <= a0, a0 + n <= nrows, 0 <= oldest < nrows.
 * dgvit_per_set_leaves: leaves [first, first + count) of the tree (inside the ring: no wrap) take leaves[k], clamped to [2^-64, 2^64]
 *   as every leaf is (a NaN gives 2^-64), and their ancestors are rebuilt as dgvit_per_set_range rebuilds them: a tree whose stored
 *   leaves are written back is bit-equal to the tree they were read from.  The max leaf (header word 0) is not an argument: it is one
 *   word of `tree` that the caller writes on the device when the last range is in.
 * Neither synchronises; both are capturable.
 * -------------------------------------------------------------------------------------------- */
typedef struct {
  const void* obs;                           /* (nrows, frame_ld) ring matrix; the arena of a shared ring */
  const void* next_obs;                      /* (next_rows, frame_ld); the arena again for a shared ring */
  const int* next_row;                       /* NULL: a two-matrix ring */
  const float* small[DGVIT_SMALL_FIELDS];    /* (nrows, small_ld[f]) fp32 */
  const unsigned char* flags;                /* may be NULL */
  const float* leaves;                       /* may be NULL */
  long long frame_ld;                        /* elements between two frame rows */
  long long next_rows;
  int small_cols[DGVIT_SMALL_FIELDS];
  int small_ld[DGVIT_SMALL_FIELDS];
  int frame_u8;
} dgvit_ring_view;
int dgvit_ring_export(dgvit_ring_view ring, void* out, long long out_bytes, long long cols, long long nrows, long long oldest, long long a0,
                      long long n, void* stream);
int dgvit_per_set_leaves(float* tree, long long capacity, long long first, long long count, const float* leaves, void* stream);

/* ----------------------------------------------------------------------------------------------
 * the depth-frame preprocessing in front of the path -- what env_lab.py does with OpenCV on the
 * host for every camera message (listener_callback :420-434: cv2.normalize MINMAX -> uint8, add_nose :78-89 (N(0, 50) noise,
 * clip, 5x5 Gaussian blur), blurring :69-76 (11x11 blur of the centre band)) and for every step (:295-299: cv2.resize to
 * 160x128, / 255).  Frames are fp32 (B, H, W) on the device; noise == NULL draws N(0, noise_level) on the device (Philox).
 * Parity against OpenCV is unpinned (cv2 is not installed in the build image; the oracle restates its published formulas).
 * -------------------------------------------------------------------------------------------- */
long long dgvit_depth_preprocess_scratch_floats(int B, int H, int W);
int dgvit_depth_to_state(const float* depth, const float* noise, float noise_level, unsigned long long seed, float* state,
                         float* scratch, long long scratch_floats, int B, int H, int W, int out_h, int out_w, void* stream);
/* the stages (operator-level tests): scratch of dgvit_depth_normalize_u8 = 128 * B floats; tmp of dgvit_gaussian_blur = B*H*W floats,
 * rows [row0, row1) are blurred (ksize 5 or 11, reflection inside the band), img may equal out */
int dgvit_depth_normalize_u8(const float* depth, float* out, float* scratch, long long scratch_floats, int B, int H, int W, void* stream);
int dgvit_noise_clip(const float* img, const float* noise, float* out, long long n, float noise_level, unsigned long long seed, void* stream);
int dgvit_gaussian_blur(const float* img, float* out, float* tmp, int B, int H, int W, int ksize, int row0, int row1, void* stream);
int dgvit_resize_bilinear(const float* img, float* out, int B, int Hs, int Ws, int Hd, int Wd, float scale, void* stream);

/* ----------------------------------------------------------------------------------------------
 * The step after the path: torch.optim.Adam.step over all tensors of a network
 * (DRL.py:401-403,412-414) and the Polyak target update target = target*(1-tau) + source*tau (utils.py:31-33),
 * each as ONE pass over flat fp32 buffers (n multiple of 4, 16-byte aligned; see dgvit_amd.optim).
 * Adam follows torch.optim.Adam: m,v updates, bias corrections with `step` (1-based), eps added to sqrt(v_hat),
 * weight_decay as L2 term added to the gradient.  step_dev (may be NULL): DEVICE pointer to the 1-based step
 * counter, overriding `step` (graph-capturable form: bias corrections are then computed in the kernel).
 * -------------------------------------------------------------------------------------------- */
int dgvit_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, long long step, const long long* step_dev, void* stream);
int dgvit_soft_update(float* target, const float* source, long long n, float tau, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Gradient-norm clipping between the backward and Adam: torch.nn.utils.clip_grad_norm_(parameters, max_norm) with norm_type 2
 * (attention_imitating.py:45-67) on the flat gradient buffers, with the norm and the coefficient left in device memory -- nothing
 * synchronises, everything is graph-capturable.  Flat buffers as above: fp32, n a positive multiple of 4, 16-byte aligned.
 *
 * dgvit_grad_sqnorm_partials: a fixed grid of DGVIT_GRAD_NORM_PARTIALS workgroups; workgroup b sums g[i]^2 over its grid-stride share
 *   in DOUBLE and stores the sum to partials[b] (accumulate == 0) or partials[b] + sum (accumulate != 0: the next buffer of the same
 *   parameter set, in stream order).  `partials`: DGVIT_GRAD_NORM_PARTIALS doubles, 16-byte aligned.  Every slot is written by the
 *   first (non-accumulating) call, so the scratch needs no memset; there are no atomics, and the result depends on the data and n only.
 * dgvit_grad_clip_coef: one workgroup sums the partials in a fixed order in double and writes
 *     out[0] = (float)sqrt(sum)                                        the total norm
 *     out[1] = min(max_norm / (out[0] + 1e-6f), 1) in fp32             the coefficient, evaluated as torch does: the reciprocal of
 *              (out[0] + 1e-6f) rounded to fp32, times max_norm, then clamp(max=1).  A NaN norm gives a NaN coefficient (torch.clamp
 *              propagates NaN), an infinite norm gives 0.  max_norm must be finite and > 0.
 * dgvit_adam_step_scaled: dgvit_adam_step on the gradient g[i] * *grad_scale_dev; the product is rounded to fp32 on its own before
 *   weight decay is added, so the result is bit-identical to dgvit_adam_step on a buffer scaled beforehand -- without writing it.
 *   grad_scale_dev (a DEVICE pointer, e.g. out + 1 of dgvit_grad_clip_coef) must not be NULL: the unscaled step is dgvit_adam_step.
 * dgvit_scale_by_device_scalar: x[i] = *scale_dev * x[i] in place (the stand-alone clip of .grad buffers).
 * -------------------------------------------------------------------------------------------- */
#define DGVIT_GRAD_NORM_PARTIALS 512
int dgvit_grad_sqnorm_partials(const float* g, long long n, double* partials, int accumulate, void* stream);
int dgvit_grad_clip_coef(const double* partials, float max_norm, float* out /* 2 floats: total norm, coefficient */, void* stream);
int dgvit_adam_step_scaled(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, long long step, const long long* step_dev,
                           const float* grad_scale_dev, void* stream);
int dgvit_scale_by_device_scalar(float* x, long long n, const float* scale_dev, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Parameter groups and learning-rate schedules: torch.optim.Adam / AdamW over ONE run of a flat buffer whose elements belong to groups
 * with their own (lr, weight_decay), with warm-up and cosine / linear decay evaluated on the device -- one launch, graph-capturable, a
 * replayed graph follows the schedule and a learning rate changed in device memory.  Flat buffers as above.
 *
 *   seg_end4 (DEVICE, nseg long longs, 8-byte aligned): the end of segment k in float4 units relative to p, strictly ascending, the last
 *     one equal to n / 4.  seg_group (DEVICE, nseg bytes): the group of segment k, < ngroups.  1 <= nseg <= 2048.
 *   group_hyper (DEVICE, 2 * ngroups floats): (lr, weight_decay) of group 0, group 1, ...  1 <= ngroups <= 256.
 *   lr_out (DEVICE, ngroups floats, may be NULL): receives lr * f per group, the learning rates this step used.
 *   step / step_dev: as dgvit_adam_step (t = *step_dev when given, else step >= 1).  The bias corrections are ALWAYS computed in the
 *     kernel, lr_t / (1 - powf(beta1, t)) and rsqrtf(1 - powf(beta2, t)), so a call with a host step and one with a device counter
 *     give the same bits.
 *   The schedule factor f, in double, rounded to fp32 once: s = (step_dev ? *step_dev : sched_step) - 1 steps were already taken;
 *     s < warmup_steps: f = (s + 1) / warmup_steps; otherwise q = min((s - warmup_steps) / max(1, total_steps - warmup_steps), 1) and
 *     sched_kind 0 (constant): f = 1     1 (cosine): f = r + (1 - r) (1 + cos(pi q)) / 2     2 (linear): f = r + (1 - r)(1 - q)
 *     with r = final_ratio in [0, 1]; past total_steps f stays r.  total_steps >= warmup_steps >= 0 (kind 0 ignores total_steps).
 *   Per element, with its group's lr_t = lr * f and wd, g first multiplied by *grad_scale_dev (may be NULL) as dgvit_adam_step_scaled does:
 *     decoupled == 0: gg = g + wd p;  m = b1 m + (1 - b1) gg;  v = b2 v + (1 - b2) gg gg;  p -= lr_c m / (sqrt(v) inv_sqrt_bc2 + eps)
 *     decoupled != 0: p = p (1 - lr_t wd) (rounded on its own), then the same lines with gg = g                       (torch.optim.AdamW)
 *   With one group, decoupled == 0 and sched_kind == 0 the result is bit-identical to dgvit_adam_step[_scaled] called with a step_dev.
 * Bad arguments (null or misaligned pointers, n, nseg, ngroups, betas outside [0, 1), step < 1 without step_dev, sched_kind,
 * warmup_steps < 0, total_steps < warmup_steps for kinds 1 and 2, final_ratio outside [0, 1]) are refused before any launch.
 * -------------------------------------------------------------------------------------------- */
int dgvit_adam_step_groups(float* p, const float* g, float* m, float* v, long long n,
                           const long long* seg_end4, const unsigned char* seg_group, int nseg,
                           const float* group_hyper, int ngroups, float* lr_out,
                           float beta1, float beta2, float eps, int decoupled,
                           long long step, long long sched_step, const long long* step_dev,
                           int sched_kind, long long warmup_steps, long long total_steps, float final_ratio,
                           const float* grad_scale_dev, void* stream);

/* ----------------------------------------------------------------------------------------------
 * The SAC loss head: the arithmetic of SAC.learn between the network forwards and the backwards (DRL.py:384-425), one launch per
 * loss with its gradient, nothing synchronises, graph-capturable.  fp32; q* are (B, A) row-major, reward / done / weights / log_pi /
 * next_log_pi hold B values; 1 <= B, 1 <= A <= 16, B * A <= 2^20.  The temperature alpha is expf(log_alpha[0]) read on the DEVICE
 * when the kernel runs (log_alpha != NULL: a replayed graph follows a learned temperature), otherwise the float `alpha`.
 * Each kernel is one workgroup that sums in double in a fixed order: no atomics, the same bits on every call.
 *
 * dgvit_sac_critic_loss:
 *     target[b,a] = reward[b] + (1 - done[b]) gamma (min(next_q1, next_q2)[b,a] - alpha next_log_pi[b])        done == NULL: 0
 *     loss[0]     = (1/BA) sum w[b] (q1 - target)^2 + (1/BA) sum w[b] (q2 - target)^2                          weights == NULL: 1
 *     td[b]       = (1/A) sum_a |q1[b,a] - target[b,a]|            (NULL: not wanted; what a prioritized replay takes back)
 *     grads       = [dq1 | dq2], 2 B A floats, d loss / d q = 2 w (q - target) / (BA) for a unit upstream gradient (NULL: not wanted)
 *   target is a constant (the reference's no_grad): nothing is produced for next_*, reward, done, weights or log_alpha.
 * dgvit_sac_critic_loss_v2: the same launch with a per-sample discount (B values, e.g. discount_out of dgvit_nstep_walk) in the place
 *   of gamma:  target[b,a] = reward[b] + (1 - done[b]) discount[b] (min(next_q1, next_q2)[b,a] - alpha next_log_pi[b]).  With
 *   discount != NULL the float gamma is not read; with discount == NULL the call IS dgvit_sac_critic_loss, bit for bit.
 * dgvit_sac_actor_loss:
 *     losses[0] = (1/BA) sum (alpha log_pi[b] - min(q1_pi, q2_pi)[b,a])                                        the policy loss
 *     grads     = [d log_pi (B) | dq1_pi (BA) | dq2_pi (BA)] (NULL: not wanted): d log_pi[b] = alpha / B; dq1_pi = -1/(BA) where
 *                 q1_pi < q2_pi, -0.5/(BA) at a tie (torch.minimum's rule), 0 otherwise; dq2_pi the mirror image
 *   and with with_temperature == 1 (needs log_alpha):
 *     losses[1]     = -log_alpha[0] (1/B) sum_b (log_pi[b] + target_entropy)                                   the temperature loss
 *     dlog_alpha[0] = -(1/B) sum_b (log_pi[b] + target_entropy)      (NULL: not wanted)
 *   `losses` holds 2 floats; losses[1] and dlog_alpha are left alone when with_temperature == 0.  The temperature loss treats log_pi
 *   as a constant and the policy loss treats log_alpha as one, so the two gradients above are all there are.
 * dgvit_sac_scale_grads: dst[i] = *scale_dev * src[i], 1 <= n <= 3 * 2^20 -- the backward of either loss: a saved gradient buffer
 *   times the 0-d upstream gradient, out of place (the saved buffer serves a second backward) and for any n and 4-byte alignment.
 * dgvit_sac_bc_loss: the demonstration term of an actor loss, normalised on the device by the rows it applies to:
 *     l[b]   = (1/A) sum_a (pred[b,a] - action[b,a])^2            nll == 0: pred and action (B, A)
 *            = -pred[b]                                            nll == 1: pred holds B log-densities, A must be 1, action is not read
 *     m[b]   = 1 (mask == NULL), mask[b] as fp32 weights >= 0 (mask_u8 == 0), or mask[b] != 0 of B bytes, a bool tensor (mask_u8 == 1)
 *     f[b]   = 1 without the four q pointers, else [ (1/A) sum_a min(q1_demo, q2_demo)[b,a] > (1/A) sum_a min(q1_pi, q2_pi)[b,a] ]
 *              (strict: a tie does not apply; the q are (B, A), given together or not at all, and not with nll == 1)
 *     out[1] = used = sum_b m[b] f[b];    out[0] = sum_b m[b] f[b] l[b] / used, or 0 when used == 0
 *     grads  = d out[0] / d pred for a unit upstream gradient, B A floats (NULL: not wanted): 2 m f (pred - action) / (A used), or
 *              -m f / used with nll; all zeros when used == 0.  A row with m f == 0 adds nothing whatever its l: never NaN from it.
 *   One workgroup, double sums in a fixed order as the two kernels above; nothing is produced for action, mask or the q.
 * dgvit_sac_cql_penalty: the conservative term of a CQL(H) critic loss over M proposal actions per row.  q1_cat, q2_cat: (B, M, C);
 *   q1_data, q2_data: (B, C); log_w: (B, M) log-density of the proposal that drew action m (NULL: 0); mask as dgvit_sac_bc_loss (m[b]).
 *     z[b,m,c] = q_cat[b,m,c] - log_w[b,m];    lse[b,c] = T log sum_m exp(z / T)   (max-subtracted, T = temperature > 0)
 *     used     = sum_b m[b];    gap_i = sum_{b,c} m[b] (lse_i[b,c] - q_data_i[b,c]) / (used C)              i = 1, 2 (the two critics)
 *     w        = exp(log_weight[0]) read on the device and taken in double (log_weight != NULL), else the float `weight`
 *     out      = [ w (gap_1 + gap_2 - 2 tau), -w (gap_1 + gap_2 - 2 tau) (lagrange == 1, else 0), gap_1, gap_2, used ]     5 floats
 *                tau = target_gap with lagrange == 1 (needs log_weight), 0 otherwise.  out[0] treats w as a constant; out[1] is the
 *                Lagrange multiplier's loss, a function of log_weight alone, and dlog_weight[0] = out[1] its derivative (NULL: not wanted)
 *     grads    = [dq1_cat (BMC) | dq2_cat (BMC) | dq1_data (BC) | dq2_data (BC)] of out[0] for a unit upstream gradient (NULL: not
 *                wanted): d q_cat = w m[b] softmax_m(z / T) / (used C), d q_data = -w m[b] / (used C); exact zeros where m[b] == 0
 *   used == 0 gives out = 0 and zero gradients, never NaN.  1 <= B, 1 <= M, 1 <= C <= 16, B (M + 1) C <= 2^20.  One workgroup, every term
 *   in double from the fp32 inputs in a fixed order; nothing is produced for log_w or mask.
 * -------------------------------------------------------------------------------------------- */
int dgvit_sac_critic_loss(const float* q1, const float* q2, const float* reward, const float* done, const float* weights,
                          const float* next_q1, const float* next_q2, const float* next_log_pi, const float* log_alpha, float alpha,
                          float gamma, float* target, float* td, float* loss, float* grads, int B, int A, void* stream);
int dgvit_sac_critic_loss_v2(const float* q1, const float* q2, const float* reward, const float* done, const float* weights,
                             const float* discount /* may be NULL */, const float* next_q1, const float* next_q2, const float* next_log_pi,
                             const float* log_alpha, float alpha, float gamma, float* target, float* td, float* loss, float* grads, int B,
                             int A, void* stream);
int dgvit_sac_actor_loss(const float* log_pi, const float* q1_pi, const float* q2_pi, const float* log_alpha, float alpha,
                         int with_temperature, float target_entropy, float* losses, float* grads, float* dlog_alpha, int B, int A,
                         void* stream);
int dgvit_sac_scale_grads(const float* src, float* dst, long long n, const float* scale_dev, void* stream);
int dgvit_sac_bc_loss(const float* pred, const float* action, const void* mask, int mask_u8, const float* q1_demo, const float* q2_demo,
                      const float* q1_pi, const float* q2_pi, int nll, float* out, float* grads, int B, int A, void* stream);
int dgvit_sac_cql_penalty(const float* q1_cat, const float* q2_cat, const float* q1_data, const float* q2_data, const float* log_w,
                          const void* mask, int mask_u8, const float* log_weight, float weight, float temperature, float target_gap,
                          int lagrange, float* out, float* grads, float* dlog_weight, int B, int M, int C, void* stream);

/* ----------------------------------------------------------------------------------------------
 * bf16 configuration (BASELINE.json config 5: 224x224 depth frames, 12-layer ViT-Base variant with goal token, bf16).
 * Same GoT.forward (GoalFormer.py:156-171) with bf16 STORAGE for every GEMM operand (LayerNorm outputs, qkv, attention
 * output, MLP hidden, the four weight matrices of each block and the patch weight) and fp32 everywhere else (residual
 * stream, LayerNorm statistics, biases, softmax, accumulation on v_mfma_f32_32x32x16_bf16, RMSNorm, output).
 * bf16 values are raw 16-bit patterns (unsigned short).  Needs dim_head 64 and dim, mlp_dim % 8 == 0; any patch size (a patch area
 * that is no multiple of 8 -- 14x14, 7x7, 3x5 -- is padded with zero columns to the next one inside the arena and the workspace, which
 * the size queries account for; parameters and gradients keep their (dim, patch pixels) shapes).
 *   wpack: bf16 copies of the GEMM weights in one arena of dgvit_got_bf16_weight_elems elements
 *          [patch weight, rows padded to a multiple of 8 | per layer: to_qkv, to_out, fc1, fc2 and their transposes], refreshed with dgvit_got_pack_weights_bf16 whenever the
 *          fp32 master parameters change; `params` is the fp32 table of dgvit_got_forward (biases, norms, pos_embedding).
 *   workspace: dgvit_got_bf16_workspace_bytes BYTES, 256-byte aligned.
 * -------------------------------------------------------------------------------------------- */
long long dgvit_got_bf16_weight_elems(const dgvit_config* cfg);
/* with_transposes == 0 fills only the (out, in) copies the forward reads (inference); != 0 also the transposes the backward's
 * data-gradient GEMMs read.  The library keeps no state: call it (on the stream of the forward) whenever the fp32 masters may
 * have changed -- the in-tree host re-packs before every forward. */
int dgvit_got_pack_weights_bf16(const dgvit_config* cfg, const float* const* params, unsigned short* wpack,
                                long long wpack_elems, int with_transposes, void* stream);
long long dgvit_got_bf16_workspace_bytes(const dgvit_config* cfg, int batch, int save_for_backward);
int dgvit_got_forward_bf16(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, const float* img,
                           const float* goal, float* feat, void* workspace, long long workspace_bytes, int batch,
                           int save_for_backward, float dropout_keep, unsigned long long dropout_seed,
                           const unsigned long long* dropout_seed_dev, void* stream);
/* Training in the bf16 configuration: forward with save_for_backward = 1 (dense last block), then
 *   dfeat (B, D) -> grads[] (fp32, table order of params, each written), dgoal (B, D) (may be NULL).
 * Gradients of GEMM operands travel bf16 (dY of every Linear), the residual-stream gradient, LayerNorm / bias / weight
 * gradients are fp32; weight gradients are fp32 split-K slabs summed in a fixed order (deterministic).
 * `img` is the forward's input (the patch-embedding weight gradient re-gathers the patches in fp32);
 * scratch: dgvit_got_bf16_backward_scratch_bytes BYTES, 256-byte aligned. */
long long dgvit_got_bf16_backward_scratch_bytes(const dgvit_config* cfg, int batch);
int dgvit_got_backward_bf16(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, float* const* grads,
                            const float* dfeat, float* dgoal, const float* img, const void* workspace, long long workspace_bytes,
                            void* scratch, long long scratch_bytes, int batch, float dropout_keep, unsigned long long dropout_seed,
                            const unsigned long long* dropout_seed_dev, void* stream);
/* ... with gradient-ready events (see dgvit_grad_events) */
int dgvit_got_backward_bf16_ev(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, float* const* grads,
                               const float* dfeat, float* dgoal, const float* img, const void* workspace, long long workspace_bytes,
                               void* scratch, long long scratch_bytes, int batch, float dropout_keep, unsigned long long dropout_seed,
                               const unsigned long long* dropout_seed_dev, void* stream, const dgvit_grad_events* events);
/* ... with the frame gradient: dimg (B, image_h, image_w) fp32, NULL = not wanted; formed in fp32 from the fp32 token-assembly gradient
 * and the fp32 master patch weight, emb-dropout mask included (as dgvit_got_backward_v3).  Same workspace and scratch sizes. */
int dgvit_got_backward_bf16_v2(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, float* const* grads,
                               const float* dfeat, float* dgoal, float* dimg, const float* img, const void* workspace,
                               long long workspace_bytes, void* scratch, long long scratch_bytes, int batch, float dropout_keep,
                               unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev, void* stream);
int dgvit_got_backward_bf16_v2_ev(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, float* const* grads,
                                  const float* dfeat, float* dgoal, float* dimg, const float* img, const void* workspace,
                                  long long workspace_bytes, void* scratch, long long scratch_bytes, int batch, float dropout_keep,
                                  unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev, void* stream,
                                  const dgvit_grad_events* events);
/* operator-level entry points of the bf16 kernels (parity tests, benches) */
/* dW (Mo, Ko) fp32 = dY^T X and db (Mo, may be NULL) = column sums of dY, for dY (T, Mo) and X (T, Ko) bf16, token-major
 * (Mo, Ko % 8 == 0): the TN layout of the ring GEMM (transposed LDS reads), split over tokens into fp32 slabs that are summed in
 * a fixed order.  scratch: dgvit_wgrad_bf16_scratch_floats floats. */
long long dgvit_wgrad_bf16_scratch_floats(int Mo, int Ko, int T);
int dgvit_wgrad_bf16(const unsigned short* dY, const unsigned short* X, float* dW, float* db, float* scratch,
                     long long scratch_floats, int T, int Mo, int Ko, void* stream);
int dgvit_cast_f32_bf16(const float* src, unsigned short* dst, long long n, void* stream);
/* C = A B^T (+ epilogue), A (M,K) / B (N,K) bf16 with k contiguous, K, lda, ldb % 8 == 0, N, ldc % 4 == 0.
 * epilogue 0: C bf16 = acc + bias;  1: C bf16 = gelu(acc + bias);  2: C fp32 = acc + bias + res (fp32);
 *          3: C bf16 = acc * gelu'(aux bf16);  4: C fp32 = acc;  5: as 1 and C2 bf16 = acc + bias (pre-activation). */
int dgvit_gemm_bf16(int epilogue, const unsigned short* A, int lda, const unsigned short* B, int ldb, void* C, int ldc, int M,
                    int N, int K, const float* bias, const float* res, int ldr, unsigned short* C2, int ldc2,
                    const unsigned short* aux, int ldaux, void* stream);
/* LayerNorm with fp32 input and bf16 output (mean / rstd may be NULL) */
int dgvit_layernorm_forward_bf16(const float* x, const float* gamma, const float* beta, unsigned short* y, float* mean,
                                 float* rstd, int rows, int D, void* stream);
/* attention core on bf16 qkv (B, N, 3*H*64) -> bf16 out (B, N, H*64); lse fp32 (B, H, N) or NULL */
int dgvit_attention_forward_bf16(const unsigned short* qkv, unsigned short* out, float* lse, int B, int N, int H, int dh,
                                 void* stream);
/* gradient of the attention core: dqkv (B, N, 3*H*64) bf16 from qkv, the forward's out and lse, and dout; delta: B*H*N floats
 * of scratch (rowsum(dout o out), handed from the dQ kernel to the dK/dV kernel) */
int dgvit_attention_backward_bf16(const unsigned short* qkv, const unsigned short* out, const unsigned short* dout, const float* lse,
                                  unsigned short* dqkv, float* delta, int B, int N, int H, int dh, void* stream);
/* The same two on the K / V-tiled kernels the bf16 encoder uses for N > 288 under DGVIT_FLAG_LONG_SEQUENCE: any N >= 1, dh = 64.
 * The forward computes the leading nq query rows (1 <= nq <= N) against every key and writes only those rows of out and lse (lse may
 * be NULL); the backward is dense and writes all B*H*N floats of delta.  Deterministic; a grid of 2^31 workgroups or more is refused. */
int dgvit_attention_forward_bf16_tiled(const unsigned short* qkv, unsigned short* out, float* lse, int B, int N, int H, int dh, int nq,
                                       void* stream);
int dgvit_attention_backward_bf16_tiled(const unsigned short* qkv, const unsigned short* out, const unsigned short* dout,
                                        const float* lse, unsigned short* dqkv, float* delta, int B, int N, int H, int dh, void* stream);
/* attention maps in the bf16 configuration (see dgvit_got_forward_maps): the arguments of dgvit_got_forward_bf16 without
 * save_for_backward, plus maps and rows */
int dgvit_got_forward_maps_bf16(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, const float* img,
                                const float* goal, float* feat, float* maps, int rows, void* workspace, long long workspace_bytes,
                                int batch, float dropout_keep, unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev,
                                void* stream);
/* probabilities from bf16 qkv (dh 64) and the lse of dgvit_attention_forward_bf16; layouts as dgvit_attention_probs */
int dgvit_attention_probs_bf16(const unsigned short* qkv, const float* lse, float* probs, int B, int N, int H, int dh, int rows,
                               void* stream);

/* Transformer-internal dropout in the bf16 configuration: the entry points above with one more argument, layer_keep in (0, 1]
 * (= 1 - GoT(dropout=p); 1.0f in eval mode), after dropout_keep.  The entry points above are these with layer_keep = 1: the same
 * launches, the same bits.  Below 1 the masks of the table at dgvit_got_forward_v2 are applied -- the same counters, keep test and
 * 1/keep scale (in fp32, before the rounding to bf16), so a bf16 and an fp32 model draw the same masks from one seed:
 *   s = 0  on the un-normalised probabilities before they are rounded to bf16 for P V; every attention call then runs on the
 *          K / V-tiled kernels, whatever N is (N > 288 still needs DGVIT_FLAG_LONG_SEQUENCE); lse stays the undropped one, so
 *          the maps of dgvit_got_forward_maps_bf16_v2 are the probabilities before the dropout
 *   s = 1, 3  on the bf16 branch output before it joins the fp32 residual stream;  s = 2  on the GELU output (the saved
 *          pre-activation is left as it is)
 * Nothing is stored; the backward regenerates every mask (pass it the forward's keeps and seed).  No buffer size changes: the
 * masked copies of the branch-output gradients live in a buffer of the scratch that is free at that point.
 * Returns DGVIT_ERR_ARG when layer_keep is outside (0, 1] (NaN included). */
int dgvit_got_forward_bf16_v2(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, const float* img,
                              const float* goal, float* feat, void* workspace, long long workspace_bytes, int batch,
                              int save_for_backward, float dropout_keep, float layer_keep, unsigned long long dropout_seed,
                              const unsigned long long* dropout_seed_dev, void* stream);
int dgvit_got_forward_maps_bf16_v2(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, const float* img,
                                   const float* goal, float* feat, float* maps, int rows, void* workspace, long long workspace_bytes,
                                   int batch, float dropout_keep, float layer_keep, unsigned long long dropout_seed,
                                   const unsigned long long* dropout_seed_dev, void* stream);
int dgvit_got_backward_bf16_v3(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, float* const* grads,
                               const float* dfeat, float* dgoal, float* dimg, const float* img, const void* workspace,
                               long long workspace_bytes, void* scratch, long long scratch_bytes, int batch, float dropout_keep,
                               float layer_keep, unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev,
                               void* stream);
int dgvit_got_backward_bf16_v3_ev(const dgvit_config* cfg, const float* const* params, const unsigned short* wpack, float* const* grads,
                                  const float* dfeat, float* dgoal, float* dimg, const float* img, const void* workspace,
                                  long long workspace_bytes, void* scratch, long long scratch_bytes, int batch, float dropout_keep,
                                  float layer_keep, unsigned long long dropout_seed, const unsigned long long* dropout_seed_dev,
                                  void* stream, const dgvit_grad_events* events);
/* operator level: the K / V-tiled bf16 attention with the site-0 mask of `layer` (keep in (0, 1]; 1 = the calls without _drop, bit
 * for bit; seed_dev, if not NULL, overrides seed at run time), and the row kernel of sites 1 - 3: dst[r][c] = src[r][c] * mask / keep
 * on `rows` rows of `width` bf16 elements (width, lds, ldd % 8 == 0, 16-byte aligned; dst may be src), buffer row r being the
 * absolute token row r * rs of a (token row, width) tensor. */
int dgvit_attention_forward_bf16_tiled_drop(const unsigned short* qkv, unsigned short* out, float* lse, int B, int N, int H, int dh,
                                            int nq, float keep, unsigned long long seed, const unsigned long long* seed_dev, int layer,
                                            void* stream);
int dgvit_attention_backward_bf16_tiled_drop(const unsigned short* qkv, const unsigned short* out, const unsigned short* dout,
                                             const float* lse, unsigned short* dqkv, float* delta, int B, int N, int H, int dh,
                                             float keep, unsigned long long seed, const unsigned long long* seed_dev, int layer,
                                             void* stream);
int dgvit_drop_rows_bf16(const unsigned short* src, long long lds, unsigned short* dst, long long ldd, long long rows, int width,
                         int rs, float keep, unsigned long long seed, const unsigned long long* seed_dev, int layer, int site,
                         void* stream);

/* ----------------------------------------------------------------------------------------------
 * Optional live kernel timing (HIP events on the launch stream around kernel launches).
 * kinds: 0 GEMM (work = 2*M*N*K FLOPs), 1 attention fwd, 2 attention bwd (work = algorithmic FLOPs),
 *        3 normalisation / reductions / elementwise (work = 0).
 * -------------------------------------------------------------------------------------------- */
#define DGVIT_PROFILE_KINDS 4
int dgvit_profile_start(int max_records);
int dgvit_profile_stop(double* ms, double* work, long long* launches);
/* Sampling (ABI 4).  An event pair around a launch keeps it from overlapping the tail of its predecessor and the ramp of its
 * successor; around EVERY launch that costs the C3 training step about 7 % (13.7 -> 14.8 ms).  dgvit_profile_sampling(s) times
 * every s-th launch of each kind only (s = 1: all; the setting persists); the sums of dgvit_profile_stop then cover the sampled
 * launches, and dgvit_profile_totals gives work and launch counts of ALL launches seen between start and stop. */
int dgvit_profile_sampling(int stride);
int dgvit_profile_totals(double* work_all, long long* launches_all);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DGVIT_HIP_H */
