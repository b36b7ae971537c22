// extern "C" surface of the CNN feature stack (dgvit_cnn_*).
#include "schedule.h"

// ---------------------------------------------------------------------------------------------- CNN feature stack
// (the shipped critic QNetwork and the CNN actor; got_sac_network.py:129-133,151-155)
namespace {
struct ConvDims {
  int B, H[4], W[4], C[4], KP[3];   // layer l maps (H[l], W[l], C[l]) -> (H[l+1], W[l+1], C[l+1])
  long long M[4];                   // rows of the NHWC activation l (M[0] unused)
};
// C: channels of the channel-last (B, H, W, C) frame stack that conv1 reads (1: single frames)
int make_conv_dims(int B, int H, int W, int C, ConvDims& d) {
  DGVIT_CHECK_ARG(B > 0 && H >= 29 && W >= 29, "cnn: need batch > 0 and frames of at least 29x29");
  DGVIT_CHECK_ARG(C >= 1 && C <= 16, "cnn: %d frame channels, need 1 to 16", C);
  d.B = B; d.H[0] = H; d.W[0] = W; d.C[0] = C; d.C[1] = 16; d.C[2] = 64; d.C[3] = 256;
  for (int l = 0; l < 3; ++l) {
    d.H[l + 1] = (d.H[l] - 5) / 2 + 1;
    d.W[l + 1] = (d.W[l] - 5) / 2 + 1;
    d.KP[l] = l == 0 && C == 1 ? 28 : (int)al4(25 * d.C[l]);   // one channel: 25 -> 28 taps; a stack: al4(25 C)
    d.M[l + 1] = (long long)B * d.H[l + 1] * d.W[l + 1];
    DGVIT_CHECK_ARG(d.H[l + 1] > 0 && d.W[l + 1] > 0 && d.M[l + 1] < (1ll << 31), "cnn: frame too small or batch too large");
  }
  return DGVIT_OK;
}
long long conv_cols_floats(const ConvDims& d) {
  long long m = 0;
  for (int l = 0; l < 3; ++l) m = std::max(m, d.M[l + 1] * d.KP[l]);
  return al4(m);
}
long long conv_wp_floats(const ConvDims& d) { return al4(16 * d.KP[0]) + al4(64 * 400) + al4(256 * 1600); }
}  // namespace

extern "C" long long dgvit_cnn_workspace_floats(int B, int H, int W) { return dgvit_cnn_workspace_floats_v2(B, H, W, 1); }
extern "C" long long dgvit_cnn_forward_scratch_floats(int B, int H, int W) { return dgvit_cnn_forward_scratch_floats_v2(B, H, W, 1); }
extern "C" long long dgvit_cnn_backward_scratch_floats(int B, int H, int W) { return dgvit_cnn_backward_scratch_floats_v2(B, H, W, 1); }

extern "C" long long dgvit_cnn_workspace_floats_v2(int B, int H, int W, int C) {
  ConvDims d;
  if (make_conv_dims(B, H, W, C, d)) return -1;
  return al4(d.M[1] * 16) + al4(d.M[2] * 64) + al4(d.M[3] * 256);
}
// split-K scratch of the forward's implicit-GEMM convolutions (conv2 / conv3; conv1 is not split)
static SplitNeed conv_split_need(const ConvDims& d) {
  SplitNeed n;
  for (int l = 1; l < 3; ++l) n.add_gather(d.M[l + 1], d.C[l + 1], d.KP[l]);
  return n;
}
static long long conv_split_floats(const ConvDims& d) {
  const SplitNeed n = conv_split_need(d);
  return n.tiles > 0 ? al4(n.tiles) + n.slab : 0;
}
extern "C" long long dgvit_cnn_forward_scratch_floats_v2(int B, int H, int W, int C) {
  ConvDims d;
  if (make_conv_dims(B, H, W, C, d)) return -1;
  return conv_cols_floats(d) + conv_wp_floats(d) + conv_split_floats(d);
}
extern "C" long long dgvit_cnn_backward_scratch_floats_v2(int B, int H, int W, int C) {
  ConvDims d;
  if (make_conv_dims(B, H, W, C, d)) return -1;
  long long dy = std::max(std::max(d.M[1] * 16, d.M[2] * 64), d.M[3] * 256);
  long long slabs = std::max(std::max(wgrad_scratch(16, d.KP[0], (int)d.M[1]), wgrad_scratch(64, 400, (int)d.M[2])), wgrad_scratch(256, 1600, (int)d.M[3]));
  return conv_cols_floats(d) + 2 * conv_wp_floats(d) + 2 * al4(dy) + slabs;
}

extern "C" int dgvit_cnn_forward(const float* img, const float* const* params, float* feat, float* ws, long long ws_floats,
                                 float* scratch, long long scratch_floats, int B, int H, int W, void* stream) {
  return dgvit_cnn_forward_v2(img, params, feat, ws, ws_floats, scratch, scratch_floats, B, H, W, 1, stream);
}

// img: the channel-last (B, H, W, C) frame stack = conv1's NHWC input
// params: conv1.weight (16,C,5,5), conv1.bias, conv2.weight (64,16,5,5), conv2.bias, conv3.weight (256,64,5,5), conv3.bias
extern "C" int dgvit_cnn_forward_v2(const float* img, const float* const* params, float* feat, float* ws, long long ws_floats,
                                    float* scratch, long long scratch_floats, int B, int H, int W, int C, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  ConvDims d;
  TRY(make_conv_dims(B, H, W, C, d));
  DGVIT_CHECK_ARG(img && params && feat && ws && scratch, "dgvit_cnn_forward: null pointer");
  for (int i = 0; i < 6; ++i) DGVIT_CHECK_ARG(params[i], "cnn parameter %d is null", i);
  if (ws_floats < dgvit_cnn_workspace_floats_v2(B, H, W, C) || scratch_floats < dgvit_cnn_forward_scratch_floats_v2(B, H, W, C))
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "dgvit_cnn_forward: workspace or scratch too small");
  float* act[4] = {nullptr, ws, ws + al4(d.M[1] * 16), ws + al4(d.M[1] * 16) + al4(d.M[2] * 64)};
  float* cols = scratch;
  float* wp[3] = {scratch + conv_cols_floats(d), nullptr, nullptr};
  wp[1] = wp[0] + al4(16 * d.KP[0]);
  wp[2] = wp[1] + al4(64 * 400);
  // in-launch split-K of the implicit-GEMM convolutions at small batches (conv3 at B = 32: 72 tiles of a 1600-deep GEMM on 256 CUs ran
  // 60 us; cut into 12 k-slices 3-4x less): arrival counters (left clean by the kernel: one memset per forward) + slabs behind the weights
  const SplitNeed csn = conv_split_need(d);
  SplitBuf csk;
  if (csn.tiles > 0) {
    csk.counters = reinterpret_cast<int*>(wp[0] + conv_wp_floats(d));
    csk.ncounters = (int)csn.tiles;
    csk.slabs = wp[0] + conv_wp_floats(d) + al4(csn.tiles);
    csk.slab_cap = csn.slab;
    TRY(zero_fill(csk.counters, (long long)sizeof(int) * csn.tiles, st));
  }
  const float* in = img;
  for (int l = 0; l < 3; ++l) {
    TRY(weight_pack(params[2 * l], wp[l], d.C[l + 1], d.C[l], d.KP[l], 0, st));
    // conv2 / conv3 (NHWC input with 16 / 64 channels): implicit GEMM - the 5x5xC windows go from the activation straight into
    // the GEMM's A tiles (the patch-gather loader with a window step of 2 C floats), no column matrix.  So does conv1 on a frame stack
    // of 4, 8, 12 or 16 channels (not split: thousands of tiles, a shallow K); with any other channel count (one channel: 25 -> 28
    // padded taps) it keeps im2col.  The backward builds the columns it needs for the weight gradients itself.
    const int C = d.C[l], pw = 5 * C;
    const int shift = 24, inv = (1 << shift) / (pw > 0 ? pw : 1) + 1;
    bool gather = g_conv_gather && C % 4 == 0 && d.KP[l] == 25 * C && ((uintptr_t)in & 15) == 0 && (long long)d.KP[l] * inv < (1ll << 32) &&
                  (long long)B * d.H[l] * d.W[l] * C < (1ll << 29);
    for (int k = 0; gather && k < d.KP[l]; ++k) gather = (int)(((unsigned long long)(unsigned)k * (unsigned)inv) >> shift) == k / pw;   // exact k / pw
    if (!gather) TRY(im2col(in, cols, B, d.H[l], d.W[l], d.C[l], d.H[l + 1], d.W[l + 1], d.KP[l], st));
    GemmParams p = gp(cols, d.KP[l], wp[l], d.KP[l], act[l + 1], d.C[l + 1], (int)d.M[l + 1], d.C[l + 1], d.KP[l]);
    p.bias = params[2 * l + 1];
    if (gather) {
      p.g_img = in; p.g_img_floats = (long long)B * d.H[l] * d.W[l] * C;
      p.g_wi = d.W[l] * C; p.g_hw = d.H[l] * d.W[l] * C; p.g_ph = 2; p.g_kh = 5; p.g_pw = pw; p.g_xs = 2 * C;
      p.g_gw = d.W[l + 1]; p.g_P = d.H[l + 1] * d.W[l + 1]; p.g_inv = inv; p.g_shift = shift;
    }
    if (gather && l > 0) csk.attach(p);
    TRY(gemm_f32(GEMM_NT, EPI_RELU, p, 1, st));   // relu(conv + bias), rows = next layer's NHWC input
    in = act[l + 1];
  }
  return avgpool(act[3], feat, B, d.H[3] * d.W[3], 256, st);
}

extern "C" int dgvit_cnn_backward(const float* img, const float* const* params, float* const* grads, const float* dfeat,
                                  const float* ws, long long ws_floats, float* scratch, long long scratch_floats, int B, int H,
                                  int W, void* stream) {
  DGVIT_CHECK_ARG(grads, "dgvit_cnn_backward: null pointer");
  for (int i = 0; i < 6; ++i) DGVIT_CHECK_ARG(grads[i], "cnn parameter/gradient %d is null", i);
  return dgvit_cnn_backward_v3(img, params, grads, dfeat, nullptr, ws, ws_floats, scratch, scratch_floats, B, H, W, 1, stream);
}

extern "C" int dgvit_cnn_backward_v2(const float* img, const float* const* params, float* const* grads, const float* dfeat, float* dimg,
                                     const float* ws, long long ws_floats, float* scratch, long long scratch_floats, int B, int H,
                                     int W, void* stream) {
  return dgvit_cnn_backward_v3(img, params, grads, dfeat, dimg, ws, ws_floats, scratch, scratch_floats, B, H, W, 1, stream);
}

// grads[i] == NULL: frozen parameter (its weight gradient is skipped); dimg != NULL: the frame gradient too (conv1's column gradient and an
// unmasked col2im onto the (B, H, W, C) frame stack)
extern "C" int dgvit_cnn_backward_v3(const float* img, const float* const* params, float* const* grads, const float* dfeat, float* dimg,
                                     const float* ws, long long ws_floats, float* scratch, long long scratch_floats, int B, int H,
                                     int W, int C, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  ConvDims d;
  TRY(make_conv_dims(B, H, W, C, d));
  DGVIT_CHECK_ARG(img && params && grads && dfeat && ws && scratch, "dgvit_cnn_backward: null pointer");
  for (int i = 0; i < 6; ++i) DGVIT_CHECK_ARG(params[i], "cnn parameter %d is null", i);
  if (ws_floats < dgvit_cnn_workspace_floats_v2(B, H, W, C) || scratch_floats < dgvit_cnn_backward_scratch_floats_v2(B, H, W, C))
    return dgvit_set_error(DGVIT_ERR_WORKSPACE, "dgvit_cnn_backward: workspace or scratch too small");
  const float* act[4] = {img, ws, ws + al4(d.M[1] * 16), ws + al4(d.M[1] * 16) + al4(d.M[2] * 64)};
  const long long dyf = al4(std::max(std::max(d.M[1] * 16, d.M[2] * 64), d.M[3] * 256));
  float* cols = scratch;
  float* wp = cols + conv_cols_floats(d);          // packed weight of the current layer (largest first)
  float* dwp = wp + conv_wp_floats(d);             // packed weight gradient
  float* dya = dwp + conv_wp_floats(d);
  float* dyb = dya + dyf;
  float* slabs = dyb + dyf;
  const long long slab_floats = scratch_floats - (slabs - scratch);
  // d(avgpool) and the ReLU of conv3
  TRY(avgpool_bwd_relu(dfeat, act[3], dya, B, d.H[3] * d.W[3], 256, st));
  float* dy = dya;
  float* dnext = dyb;
  for (int l = 2; l >= 0; --l) {
    const int cout = d.C[l + 1], KP = d.KP[l];
    const int M = (int)d.M[l + 1];
    if (grads[2 * l] || grads[2 * l + 1]) {
      TRY(im2col(act[l], cols, B, d.H[l], d.W[l], d.C[l], d.H[l + 1], d.W[l + 1], KP, st));
      TRY(wgrad(dy, cout, cols, KP, grads[2 * l] ? dwp : nullptr, grads[2 * l + 1], cout, KP, M, slabs, slab_floats, st));
      if (grads[2 * l]) TRY(weight_pack(dwp, grads[2 * l], cout, d.C[l], KP, 1, st));
    }
    if (l == 0 && dimg) {
      // conv1: dcols (M1 x KP) = dy W1 (the padded taps' weights are zero), then each pixel sums the <= 9 windows that cover it -- no
      // ReLU mask, the frame is an input
      TRY(weight_pack(params[0], wp, cout, C, KP, 0, st));
      GemmParams p = gp(dy, cout, wp, KP, cols, KP, M, KP, cout);
      TRY(gemm_f32(GEMM_NN, EPI_STORE, p, 1, st));
      TRY(col2im_frame(cols, dimg, B, H, W, C, d.H[1], d.W[1], KP, st));
    }
    if (l > 0) {
      TRY(weight_pack(params[2 * l], wp, cout, d.C[l], KP, 0, st));
      GemmParams p = gp(dy, cout, wp, KP, cols, KP, M, KP, cout);   // dcols = dy W  (cols buffer reused)
      TRY(gemm_f32(GEMM_NN, EPI_STORE, p, 1, st));
      TRY(col2im_relu(cols, act[l], dnext, B, d.H[l], d.W[l], d.C[l], d.H[l + 1], d.W[l + 1], st));
      float* t = dy; dy = dnext; dnext = t;
    }
  }
  return DGVIT_OK;
}
