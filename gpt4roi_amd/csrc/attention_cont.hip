// attention_cont.hip -- causal attention of a SHORT query block against a LONG KV cache, keys split over workgroups.
//
//   The follow-up turn of a conversation (gpt4roi/app.py keeps `history_cache` and re-sends it): the cache already holds the
//   keys and values of the earlier turns, the new tokens are 2-64 query rows that attend 800-2000 cached rows.  The prefill
//   forward (attention.hip / attention_v2.hip) launches ceil(Tq / 64) x H workgroups for that shape -- 32 on 256 CUs -- and
//   each walks every key tile serially.  attn_decode splits the keys of ONE query row over workgroups; this is the same idea
//   for a block of query rows, on MFMA:
//     * grid (splits, H, B).  Split s owns the key tiles [s * tps, (s + 1) * tps) of the ceil(Tk / 64) tiles of 64 keys,
//       tps = ceil(tiles / splits); a split past the last tile leaves an empty partial (m = -inf, l = 0).
//     * a workgroup = 2 waves x 32 query rows (Tq <= 64: the whole Q block stays in registers as the MFMA B operand); the
//       tile loop is the first form's (attention.hip): K row-major swizzled and V transposed in LDS, staged through
//       registers one tile ahead, S^T = K Q^T and O^T += V^T P^T with v_mfma_f32_32x32x16, a lane owns one query row's
//       online-softmax state.  P enters the PV product as a 16-bit value plus its 16-bit residual (two MFMAs).  A wave
//       whose 32 rows lie beyond Tq only helps staging.
//     * each split leaves the un-normalised fp32 partial (acc [64][D], m [64], l [64]; log2 domain) of its query rows in
//       the caller's workspace; a second small launch merges the splits per (row, head) and stores the 16-bit output.  Two
//       launches instead of an arrival counter: the kernel boundary publishes the partials, nothing has to be re-armed,
//       and the merge runs on Tq x H / 2 workgroups instead of on the last one to arrive.
//   Causal rule as everywhere: query i sees keys <= i + (Tk - Tq).
#include "g4r_common.h"

namespace {

constexpr int C_KVB = 64;        // keys per tile
constexpr int C_VT_LD = 68;      // Vt row stride in elements (136 B: conflict-free ds_read_b64)
constexpr int C_QB = 64;         // query rows per workgroup = the most the entry point takes

struct ContArgs {
  const h16_t* Q;
  const h16_t* K;
  const h16_t* V;
  h16_t* O;
  float* ws;                             // [B][H][S][C_QB * (D + 2)]: acc [C_QB][D], m [C_QB], l [C_QB]
  long q_row, k_row, v_row, o_row;       // row strides (elements)
  long q_batch, k_batch, v_batch, o_batch;
  int Tq, Tk, H, S;
  float scale;
};

template <int D>
__device__ __forceinline__ int c_swz(int row) {
  return D == 128 ? (row & 15) : ((row >> 1) & 7);
}

template <int D>
__global__ __launch_bounds__(128) void attn_cont_split_kernel(ContArgs p) {
  constexpr int NT = 128;
  constexpr int SLOTS = D / 8;            // 16-B slots per key row
  constexpr int KSTEPS = D / 16;          // MFMA k-steps over the head dim
  constexpr int DB = D / 32;              // 32-row blocks of O^T
  constexpr int NK = C_KVB * SLOTS / NT;  // K slots staged per thread
  constexpr int NVU = 16 * SLOTS / NT;    // V units (4 keys x one 8-wide d slot) per thread
  static_assert(C_KVB * SLOTS % NT == 0 && 16 * SLOTS % NT == 0, "staging split");
  __shared__ __attribute__((aligned(16))) h16_t Ks[C_KVB * D];
  __shared__ __attribute__((aligned(16))) h16_t Vt[D * C_VT_LD];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, ql = lane & 31;
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int qi = wave * 32 + ql;
  const int off = p.Tk - p.Tq;
  const bool wave_on = wave * 32 < p.Tq;       // wave-uniform: this wave has query rows
  const h16_t* Qb = p.Q + (size_t)b * p.q_batch + (size_t)h * D;
  const h16_t* Kb = p.K + (size_t)b * p.k_batch + (size_t)h * D;
  const h16_t* Vb = p.V + (size_t)b * p.v_batch + (size_t)h * D;

  // Q fragments (B operand: lane holds Q[q = lane&31][d = kk*16 + hi*8 .. +7]); rows beyond Tq re-read the last row
  h16x8 qf[KSTEPS];
  {
    const int qr = qi < p.Tq ? qi : p.Tq - 1;
    const h16_t* qrow = Qb + (size_t)qr * p.q_row + hi * 8;
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) qf[kk] = *reinterpret_cast<const h16x8*>(qrow + kk * 16);
  }

  float16v oacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float sc2 = p.scale * 1.4426950408889634f;  // scores are kept as s*scale*log2(e)

  // this split's keys: whole tiles, the last one cut at Tk (the last query row sees every key: no causal cut of the range)
  const int ntiles = (p.Tk + C_KVB - 1) / C_KVB;
  const int tps = (ntiles + p.S - 1) / p.S;
  const int jbegin = s * tps * C_KVB;
  int kend = (s + 1) * tps * C_KVB;
  if (kend > p.Tk) kend = p.Tk;

  uint4v kreg[NK], vreg[NVU][4];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int it = 0; it < NK; ++it) {
      const int pk = it * NT + tid;
      const int row = pk / SLOTS, sl = pk % SLOTS;
      int key = j0 + row;
      if (key > p.Tk - 1) key = p.Tk - 1;
      kreg[it] = *reinterpret_cast<const uint4v*>(Kb + (size_t)key * p.k_row + sl * 8);
    }
#pragma unroll
    for (int u = 0; u < NVU; ++u) {
      const int pu = u * NT + tid;
      const int kq = pu % 16, vs = pu / 16;   // key quad, d slot
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int key = j0 + kq * 4 + j;
        if (key > p.Tk - 1) key = p.Tk - 1;
        vreg[u][j] = *reinterpret_cast<const uint4v*>(Vb + (size_t)key * p.v_row + vs * 8);
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < NK; ++it) {
      const int pk = it * NT + tid;
      const int row = pk / SLOTS, sl = pk % SLOTS;
      *reinterpret_cast<uint4v*>(reinterpret_cast<char*>(Ks) + row * (D * 2) + ((sl ^ c_swz<D>(row)) << 4)) = kreg[it];
    }
    // V^T: this thread holds 4 consecutive keys x 8 d values -> for each d one 8-byte store of 4 keys
#pragma unroll
    for (int u = 0; u < NVU; ++u) {
      const int pu = u * NT + tid;
      const int kq = pu % 16, vs = pu / 16;
      const unsigned w[4][4] = {{vreg[u][0].x, vreg[u][0].y, vreg[u][0].z, vreg[u][0].w},
                                {vreg[u][1].x, vreg[u][1].y, vreg[u][1].z, vreg[u][1].w},
                                {vreg[u][2].x, vreg[u][2].y, vreg[u][2].z, vreg[u][2].w},
                                {vreg[u][3].x, vreg[u][3].y, vreg[u][3].z, vreg[u][3].w}};
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // word e holds d = 2e (low half) and 2e+1 (high half)
        const uint2v lo = {(w[0][e] & 0xffffu) | (w[1][e] << 16), (w[2][e] & 0xffffu) | (w[3][e] << 16)};
        const uint2v hi2 = {(w[0][e] >> 16) | (w[1][e] & 0xffff0000u), (w[2][e] >> 16) | (w[3][e] & 0xffff0000u)};
        *reinterpret_cast<uint2v*>(Vt + (vs * 8 + 2 * e) * C_VT_LD + kq * 4) = lo;
        *reinterpret_cast<uint2v*>(Vt + (vs * 8 + 2 * e + 1) * C_VT_LD + kq * 4) = hi2;
      }
    }
  };

  if (jbegin < kend) fetch(jbegin);
  for (int j0 = jbegin; j0 < kend; j0 += C_KVB) {
    commit();
    __syncthreads();
    if (j0 + C_KVB < kend) fetch(j0 + C_KVB);  // in flight during this tile's MFMAs

    // a wave without query rows, or whose 32 rows all lie above the tile's first key, has nothing to add (wave-uniform)
    if (wave_on && j0 <= wave * 32 + 31 + off) {
      // ---- S^T = K Q^T for two 32-key blocks ----
      float16v sacc[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
        const int row = kb * 32 + ql;
        const char* krow = reinterpret_cast<const char*>(Ks) + row * (D * 2);
        const int sw = c_swz<D>(row);
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) {
          const h16x8 kf = *reinterpret_cast<const h16x8*>(krow + (((kk * 2 + hi) ^ sw) << 4));
          sacc[kb] = G4R_MFMA_32X32X16(kf, qf[kk], sacc[kb], 0, 0, 0);
        }
      }

      // ---- online softmax for this lane's query (keys: j0 + kb*32 + (r&3) + 8*(r>>2) + 4*hi), log2 domain ----
      const bool need_mask = (j0 + C_KVB > p.Tk) || (j0 + C_KVB - 1 > wave * 32 + off);
      float mt = -INFINITY;
      if (need_mask) {  // wave-uniform: only the diagonal / last tiles pay for the per-key tests
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = j0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            float sv = sacc[kb][r] * sc2;
            if (key >= p.Tk || key > qi + off) sv = -INFINITY;
            sacc[kb][r] = sv;
            mt = fmaxf(mt, sv);
          }
      } else {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            sacc[kb][r] *= sc2;
            mt = fmaxf(mt, sacc[kb][r]);
          }
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32));
      const float m_new = fmaxf(m_run, mt);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;  // fully masked so far: 2^(-inf - 0) = 0
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);  // m_run = -inf -> 0
      float rs = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = __builtin_amdgcn_exp2f(sacc[kb][r] - m_use);
          sacc[kb][r] = e;
          rs += e;
        }
      rs += __shfl_xor(rs, 32);
      l_run = l_run * alpha + rs;
      m_run = m_new;
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;

      // ---- O^T += V^T P^T, P as a 16-bit value plus its 16-bit rounding residual (two MFMAs per V fragment): the one
      //      rounding the prefill forward applies to P is the largest term of its error, and with it the merged splits
      //      missed the 1.25x error margin against the forward (tests/test_attention_cont_gpu.py).  The second MFMA
      //      doubles the PV issue; its cost has not been measured on its own ----
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          unsigned ph[4], pl[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float a = sacc[kb][hf * 8 + 2 * e], c = sacc[kb][hf * 8 + 2 * e + 1];
            ph[e] = pack_h16x2(a, c);
            pl[e] = pack_h16x2(a - h16lo(ph[e]), c - h16hi(ph[e]));
          }
          const uint4v pwh = {ph[0], ph[1], ph[2], ph[3]}, pwl = {pl[0], pl[1], pl[2], pl[3]};
          const h16x8 pf = __builtin_bit_cast(h16x8, pwh), pr = __builtin_bit_cast(h16x8, pwl);
          const int kbase = kb * 32 + hf * 16 + 4 * hi;
#pragma unroll
          for (int d = 0; d < DB; ++d) {
            const h16_t* vrow = Vt + (d * 32 + ql) * C_VT_LD + kbase;
            const uint2v lo = *reinterpret_cast<const uint2v*>(vrow);
            const uint2v hi2 = *reinterpret_cast<const uint2v*>(vrow + 8);
            const uint4v vw = {lo.x, lo.y, hi2.x, hi2.y};
            const h16x8 vf = __builtin_bit_cast(h16x8, vw);
            oacc[d] = G4R_MFMA_32X32X16(vf, pf, oacc[d], 0, 0, 0);
            oacc[d] = G4R_MFMA_32X32X16(vf, pr, oacc[d], 0, 0, 0);
          }
        }
    }
    __syncthreads();
  }

  // ---- the un-normalised partial of this split: lane owns query qi, d = db*32 + 8*g + 4*hi + (0..3) ----
  if (qi < p.Tq) {
    float* base = p.ws + (((size_t)b * p.H + h) * p.S + s) * (size_t)(C_QB * (D + 2));
    float* arow = base + (size_t)qi * D;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4v w = {oacc[d][g * 4], oacc[d][g * 4 + 1], oacc[d][g * 4 + 2], oacc[d][g * 4 + 3]};
        *reinterpret_cast<float4v*>(arow + d * 32 + g * 8 + 4 * hi) = w;
      }
    if (hi == 0) {
      base[C_QB * D + qi] = m_run;
      base[C_QB * D + C_QB + qi] = l_run;
    }
  }
}

// One (query row, head) per D / 4 lanes: out = sum_s 2^(m_s - m) acc_s / sum_s 2^(m_s - m) l_s, in split order.
template <int D>
__global__ __launch_bounds__(64) void attn_cont_merge_kernel(ContArgs p) {
  constexpr int TPR = D / 4, RPB = 64 / TPR;
  constexpr size_t BLK = (size_t)C_QB * (D + 2);
  const int row = blockIdx.x * RPB + threadIdx.x / TPR, c = threadIdx.x % TPR;
  const int h = blockIdx.y, b = blockIdx.z;
  if (row >= p.Tq) return;
  const float* base = p.ws + ((size_t)b * p.H + h) * p.S * BLK;
  float mm = -INFINITY;
  for (int s = 0; s < p.S; ++s) mm = fmaxf(mm, base[s * BLK + C_QB * D + row]);
  float L = 0.f;
  float4v acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.S; ++s) {
    const float* part = base + s * BLK;
    const float ms = part[C_QB * D + row];
    if (ms == -INFINITY) continue;                 // an empty split, or one this row sees no key of
    const float w = __builtin_amdgcn_exp2f(ms - mm);
    L += w * part[C_QB * D + C_QB + row];
    const float4v a = *reinterpret_cast<const float4v*>(part + (size_t)row * D + c * 4);
    acc += a * w;
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  const uint2v o = {pack_h16x2(acc.x * inv, acc.y * inv), pack_h16x2(acc.z * inv, acc.w * inv)};
  *reinterpret_cast<uint2v*>(p.O + (size_t)b * p.o_batch + (size_t)row * p.o_row + (size_t)h * D + c * 4) = o;
}

}  // namespace

extern "C" {

// Q [B][Tq][...], 1 <= Tq <= 64; K/V [B][>= Tk][...] cache views, Tk >= Tq; O [B][Tq][...]; 16-bit; strides in elements.
// workspace: B * H * splits * 64 * (head_dim + 2) floats owned by the caller (no state survives the call).
int g4r_flash_attn_cont_bf16(const void* Q, const void* K, const void* V, void* O, float* workspace, long workspace_floats,
                             int B, int H, int Tq, int Tk, int head_dim, long q_row, long k_row, long v_row, long o_row,
                             long q_batch, long k_batch, long v_batch, long o_batch, float scale, int splits,
                             void* stream) {
  G4R_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535, "flash_attn_cont: bad shape");
  G4R_REQUIRE(Tq >= 1 && Tq <= C_QB, "flash_attn_cont: 1 <= Tq <= 64 (longer query blocks are the prefill forward's)");
  G4R_REQUIRE(Tk >= Tq, "flash_attn_cont: causal needs Tk >= Tq");
  G4R_REQUIRE(head_dim == 64 || head_dim == 128, "flash_attn_cont: head_dim must be 64 or 128");
  G4R_REQUIRE(Q && K && V && O && workspace, "flash_attn_cont: null pointer");
  G4R_REQUIRE(splits >= 1 && splits <= 64, "flash_attn_cont: splits must be in [1, 64]");
  G4R_REQUIRE(workspace_floats >= (long)B * H * splits * C_QB * (head_dim + 2), "flash_attn_cont: workspace too small");
  G4R_REQUIRE(((uintptr_t)workspace & 15) == 0, "flash_attn_cont: the workspace must be 16-byte aligned");
  G4R_REQUIRE((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V) & 15) == 0 && ((uintptr_t)O & 7) == 0,
              "flash_attn_cont: Q, K, V must be 16-byte aligned and O 8-byte aligned");
  G4R_REQUIRE(q_row % 8 == 0 && k_row % 8 == 0 && v_row % 8 == 0 && o_row % 4 == 0 && q_batch % 8 == 0 &&
                  k_batch % 8 == 0 && v_batch % 8 == 0 && o_batch % 4 == 0,
              "flash_attn_cont: strides must keep 16-byte alignment");
  ContArgs a = {(const h16_t*)Q, (const h16_t*)K, (const h16_t*)V, (h16_t*)O, workspace, q_row, k_row, v_row, o_row,
                q_batch, k_batch, v_batch, o_batch, Tq, Tk, H, splits, scale};
  hipStream_t st = (hipStream_t)stream;
  if (head_dim == 64) {
    hipLaunchKernelGGL((attn_cont_split_kernel<64>), dim3(splits, H, B), dim3(128), 0, st, a);
    hipLaunchKernelGGL((attn_cont_merge_kernel<64>), dim3(g4r_ceil_div(Tq, 4), H, B), dim3(64), 0, st, a);
  } else {
    hipLaunchKernelGGL((attn_cont_split_kernel<128>), dim3(splits, H, B), dim3(128), 0, st, a);
    hipLaunchKernelGGL((attn_cont_merge_kernel<128>), dim3(g4r_ceil_div(Tq, 2), H, B), dim3(64), 0, st, a);
  }
  G4R_CHECK_LAUNCH("flash_attn_cont");
  return G4R_OK;
}

}  // extern "C"
