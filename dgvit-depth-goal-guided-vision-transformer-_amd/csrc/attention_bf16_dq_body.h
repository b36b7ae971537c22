// The body of the two dQ kernels of attention_bf16_long.hip (attn_bwd_dq_bf16_tiled_kernel, ..._drop_kernel), included into each with
// `DROP` (constexpr bool) and `drop` (LayerDrop) in scope.  Textual inclusion for the reason given in attention_bf16_dkv_body.h: behind
// an inlined call the 4-wave instantiation without dropout moved 16 registers from VGPRs to AGPRs.
  constexpr int DH = 64, LQ = 32 * NW, STAGE = 2 * TILE + TILE_T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int nqb = (N + LQ - 1) / LQ;
  const int item = blockIdx.x / nqb, qb = blockIdx.x % nqb;
  const int b = item / H, hd = item % H;
  const int I = H * DH;
  const long long ld = 3ll * I;
  const bf16_t* base = qkv + (long long)b * N * ld + hd * DH;
  const float sc = scale * DGVIT_LOG2E;
  const int q = qb * LQ + wave * 32 + li, qc = q < N ? q : 0;
  const bool active = qb * LQ + wave * 32 < N;
  const bool fetcher = tid < FETCHERS;
  const int nkt = (N + 31) / 32, ntile = (N + LK - 1) / LK;

  bf16x8 qf[4], dof[4];
  float dl = 0.f;
  {
    bf16x8 of[4];
    load_frags(qf, base + qc * ld, h);
    load_frags(dof, d_out + ((long long)b * N + qc) * I + hd * DH, h);
    load_frags(of, o_fwd + ((long long)b * N + qc) * I + hd * DH, h);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) dl += (float)dof[s][j] * (float)of[s][j];
    dl += __shfl_xor(dl, 32, 64);
  }
  const float lq = lse[((long long)b * H + hd) * N + qc];
  if (active && q < N && h == 0) delta[((long long)b * H + hd) * N + q] = dl;
  RowDrop rd = {};
  if constexpr (DROP) rd = RowDrop{(((long long)b * H + hd) * N + qc) * ((N + 3) / 4), drop_seed(drop), drop.tag, drop.keep, 1.0f / drop.keep};

  TileRegs kr, vr;
  auto fetch = [&](int t) {
    kr.fetch(base + I, ld, t * LK, N, tid);
    vr.fetch(base + 2 * I, ld, t * LK, N, tid);
  };
  auto stash = [&](int t) {
    unsigned char* st = smem + (t & 1) * STAGE;
    kr.stash_rows<false>(st, tid);
    vr.stash_rows<false>(st + TILE, tid);
    kr.stash_transposed(reinterpret_cast<bf16_t*>(st + 2 * TILE), tid);
  };
  if (fetcher) {
    fetch(0);
    stash(0);
  }
  __syncthreads();

  f32x16 dq[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dq[0][r] = 0.f;
    dq[1][r] = 0.f;
  }
#pragma unroll 1
  for (int t = 0; t < ntile; ++t) {
    if (fetcher && t + 1 < ntile) fetch(t + 1);
    const unsigned char* Ks = smem + (t & 1) * STAGE;
    const unsigned char* Vs = Ks + TILE;
    const bf16_t* Kt = reinterpret_cast<const bf16_t*>(Ks + 2 * TILE);
    if (active) {
#pragma unroll 1
      for (int sub = 0; sub < 2; ++sub) {
        const int kt = 2 * t + sub;
        if (kt >= nkt) break;   // wave-uniform: an odd last tile
        f32x16 s0, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] = 0.f;
          dp[r] = 0.f;
        }
        mfma_rows(s0, Ks, sub * 32, li, h, qf);
        mfma_rows(dp, Vs, sub * 32, li, h, dof);
        if constexpr (DROP) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float f[4];
            rd.factors(kt * 8 + 2 * g + h, f);
#pragma unroll
            for (int i = 0; i < 4; ++i) dp[4 * g + i] *= f[i];
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + acc_row(r, h);
          const float pr = key < N ? __builtin_amdgcn_exp2f(s0[r] * sc - lq) : 0.f;
          s0[r] = pr * (dp[r] - dl) * scale;   // dS^T
        }
        mfma_transposed(dq, Kt, VS, sub * 32, li, h, s0);
      }
    }
    if (fetcher && t + 1 < ntile) stash(t + 1);
    __syncthreads();
  }
  if (active && q < N) store_T_bf16(dq, dqkv + ((long long)b * N + q) * ld + hd * DH, h, 1.f);
