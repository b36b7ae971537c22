// The body of the two dK / dV kernels of attention_bf16_long.hip (attn_bwd_dkv_bf16_tiled_kernel, ..._drop_kernel), included into
// each with `DROP` (constexpr bool) and `drop` (LayerDrop) in scope.  Textual inclusion, not a shared __device__ function: behind an
// inlined call the register allocation of the kernel without dropout changed (206 instead of 203 VGPRs), and that kernel is to stay
// the code it was.
  constexpr int DH = 64, LQ = 32 * NW, STAGE = 2 * TILE + 2 * TILE_T + 2 * LK * 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int nkb = (N + LQ - 1) / LQ;
  const int item = blockIdx.x / nkb, kb = blockIdx.x % nkb;
  const int b = item / H, hd = item % H;
  const int I = H * DH;
  const long long ld = 3ll * I;
  const bf16_t* base = qkv + (long long)b * N * ld + hd * DH;
  const bf16_t* dob = d_out + (long long)b * N * I + hd * DH;
  const float* lbase = lse + ((long long)b * H + hd) * N;
  const float* dbase = delta + ((long long)b * H + hd) * N;
  const float sc = scale * DGVIT_LOG2E;
  const int key = kb * LQ + wave * 32 + li, kc = key < N ? key : 0;
  const bool kvalid = key < N;
  const bool active = kb * LQ + wave * 32 < N;   // wave-uniform: this wave's key tile holds a real key
  const bool fetcher = tid < FETCHERS;
  const int nqt = (N + 31) / 32, ntile = (N + LK - 1) / LK;

  // mask element (q, key): float4 group ((b*H + hd)*N + q) * n4 + key / 4, word key % 4
  long long n4 = 0, dg0 = 0;
  unsigned long long dseed = 0ull;
  float dinv = 1.f;
  if constexpr (DROP) {
    n4 = (N + 3) / 4;
    dg0 = ((long long)b * H + hd) * N * n4 + (key >> 2);   // (key, not kc: the four lanes of a quad must name one group, see below)
    dseed = drop_seed(drop);
    dinv = 1.0f / drop.keep;
  }
  bf16x8 kf[4], vf[4];
  load_frags(kf, base + I + kc * ld, h);
  load_frags(vf, base + 2 * I + kc * ld, h);
  // the row statistics of a query tile travel with its Q / dO rows: the first 64 threads load one each
  TileRegs qr, dor;
  float ls = 0.f, ds = 0.f;
  auto fetch = [&](int t) {
    qr.fetch(base, ld, t * LK, N, tid);
    dor.fetch(dob, (long long)I, t * LK, N, tid);
    if (tid < LK) {
      const int r = t * LK + tid;
      ls = r < N ? lbase[r] : 0.f;
      ds = r < N ? dbase[r] : 0.f;
    }
  };
  auto stash = [&](int t) {
    unsigned char* st = smem + (t & 1) * STAGE;
    qr.stash_rows<false>(st, tid);
    dor.stash_rows<false>(st + TILE, tid);
    qr.stash_transposed(reinterpret_cast<bf16_t*>(st + 2 * TILE), tid);
    dor.stash_transposed(reinterpret_cast<bf16_t*>(st + 2 * TILE + TILE_T), tid);
    if (tid < LK) {
      float* stat = reinterpret_cast<float*>(st + 2 * TILE + 2 * TILE_T);
      stat[tid] = ls;
      stat[LK + tid] = ds;
    }
  };
  if (fetcher) {
    fetch(0);
    stash(0);
  }
  __syncthreads();

  f32x16 dk[2], dv[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f;
  }
#pragma unroll 1
  for (int t = 0; t < ntile; ++t) {
    if (fetcher && t + 1 < ntile) fetch(t + 1);
    const unsigned char* Qs = smem + (t & 1) * STAGE;
    const unsigned char* Os = Qs + TILE;                                     // dO rows
    const bf16_t* Qt = reinterpret_cast<const bf16_t*>(Qs + 2 * TILE);
    const bf16_t* Ot = reinterpret_cast<const bf16_t*>(Qs + 2 * TILE + TILE_T);   // dO transposed
    const float* lse_s = reinterpret_cast<const float*>(Qs + 2 * TILE + 2 * TILE_T);
    const float* del_s = lse_s + LK;
    if (active) {
#pragma unroll 1
      for (int sub = 0; sub < 2; ++sub) {
        const int qt = 2 * t + sub;
        if (qt >= nqt) break;   // wave-uniform: an odd last tile
        f32x16 s0, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] = 0.f;
          dp[r] = 0.f;
        }
        mfma_rows(s0, Qs, sub * 32, li, h, kf);     // S[query][key]: queries in the registers, key on the lane
        mfma_rows(dp, Os, sub * 32, li, h, vf);     // dP = dO V^T
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ql = sub * 32 + 8 * g + 4 * h, q0 = t * LK + ql;   // registers 4g .. 4g+3 hold queries q0 .. q0+3
          const fx4 l4 = *reinterpret_cast<const fx4*>(lse_s + ql), d4 = *reinterpret_cast<const fx4*>(del_s + ql);
          // The Philox block of (query, key / 4) holds the words of FOUR keys, and those keys sit on the four lanes of one quad: lane w of
          // the quad draws the block of query q0 + w alone and packs its four keep decisions into bits 0 .. 3; quad broadcasts (DPP
          // quad_perm, all lanes active: this is wave-uniform code) hand every lane the nibble of each query, of which it reads bit
          // key % 4.  One Philox call per four registers, as in the other two kernels, instead of one per register.
          int keep4[4] = {0, 0, 0, 0};
          if constexpr (DROP) {
            const uint4 rb = drop_bits(dg0 + (q0 + (lane & 3)) * n4, dseed, drop.tag);
            const int nib = (drop_factor(rb.x, drop.keep, 1.f) != 0.f ? 1 : 0) | (drop_factor(rb.y, drop.keep, 1.f) != 0.f ? 2 : 0) |
                            (drop_factor(rb.z, drop.keep, 1.f) != 0.f ? 4 : 0) | (drop_factor(rb.w, drop.keep, 1.f) != 0.f ? 8 : 0);
            keep4[0] = __builtin_amdgcn_update_dpp(0, nib, 0x00, 0xF, 0xF, false);   // quad_perm [0, 0, 0, 0]
            keep4[1] = __builtin_amdgcn_update_dpp(0, nib, 0x55, 0xF, 0xF, false);   // quad_perm [1, 1, 1, 1]
            keep4[2] = __builtin_amdgcn_update_dpp(0, nib, 0xAA, 0xF, 0xF, false);   // quad_perm [2, 2, 2, 2]
            keep4[3] = __builtin_amdgcn_update_dpp(0, nib, 0xFF, 0xF, 0xF, false);   // quad_perm [3, 3, 3, 3]
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * g + i;
            const float pr = (kvalid && q0 + i < N) ? __builtin_amdgcn_exp2f(s0[r] * sc - l4[i]) : 0.f;
            if constexpr (DROP) {
              const float f = ((keep4[i] >> (lane & 3)) & 1) ? dinv : 0.f;
              s0[r] = pr * f;                                // P o mask / keep
              dp[r] = pr * (f * dp[r] - d4[i]) * scale;      // dS
            } else {
              s0[r] = pr;                                // P
              dp[r] = pr * (dp[r] - d4[i]) * scale;      // dS
            }
          }
        }
        mfma_transposed(dv, Ot, VS, sub * 32, li, h, s0);   // dV^T += dO^T P
        mfma_transposed(dk, Qt, VS, sub * 32, li, h, dp);   // dK^T += Q^T dS
      }
    }
    if (fetcher && t + 1 < ntile) stash(t + 1);
    __syncthreads();
  }
  if (active && kvalid) {
    store_T_bf16(dk, dqkv + ((long long)b * N + key) * ld + I + hd * DH, h, 1.f);
    store_T_bf16(dv, dqkv + ((long long)b * N + key) * ld + 2 * I + hd * DH, h, 1.f);
  }
