// attention_shared.hip -- one decode step for B sequences whose first P cache rows hold the SAME tokens (one image, many
// questions; several samples of one prompt).  attn_decode_kernel (attention.hip) runs one workgroup set per (sequence,
// head), so the prefix K/V is streamed once per sequence; here it is streamed once per (head, key split) for a GROUP of up
// to 16 sequences, the way the batch already shares the weight stream.
//
//   grid (S key splits, H heads, ceil(B / 16) row groups), 4 waves.
//   Row b attends   keys [0, P) of cache slot 0  (prefix phase, shared)
//                 + keys [P, len_b) of slot b    (own phase, per row)
//                 + its own new key              (from registers, appended at row len_b of slot b).
//   * RoPE of the new q / k rows at position len_b and the cache append: the expressions and 16-bit roundings of
//     attn_decode_kernel's fused path (= rope_qkv_kernel), so the appended rows are bit-equal to that kernel's.  The rotated
//     q rows of the group (16-bit), the new k and v rows wait in LDS.
//   * Prefix phase, on the matrix pipe: the 32-key tiles of [0, P) are dealt round-robin to the 4 S wave-units (split s, wave
//     w takes tiles 4 s + w, 4 s + w + 4 S, ...: a function of P and S only).  S^T = K Q^T with v_mfma_f32_16x16x32: the K
//     rows come straight from memory as the A operand (lane = key, 16 B of the head dim), the <= 16 query rows are the B
//     operand, so a lane owns ONE query column (its scores, running max, sum, O^T registers).  O^T += V^T P^T: V goes
//     row-major through a wave-private LDS tile and comes back as the A operand by ds_read_b64_tr_b16 (attention_v2.hip);
//     the key order inside the 32-key step is permuted to the order the lane already holds P in (no shuffle of P).
//     P enters that product as a 16-bit value plus its 16-bit rounding residual (two MFMAs), as in attention_cont.hip.
//   * Own phase, the form of attn_decode_kernel: a wave takes rows w, w + 4, ... of the group, 16 B per lane, fp32 p.
//   * The 4 prefix partials and the own partial of every row are merged through LDS into one un-normalised (m, l, o[D]) per
//     (row, head, split); splits meet through `ws` and the LAST workgroup of a (group, head) to arrive merges them and
//     re-arms the counter: the hand-off of attn_decode_kernel (write-through stores, drained, relaxed agent-scope counter).
//     No workgroup waits for another; the workspace carries nothing from call to call.
//   A row's arithmetic depends on (P, len_b, S) and its own operands only: not on which rows share the launch, nor on its
//   index among them (an MFMA output column depends on its own operand column alone).
#include "g4r_common.h"

namespace {

struct SharedAttnArgs {
  const h16_t* qkv;    // [B][3 * H * D] raw q | k | v rows of the new tokens
  const float* cs;     // cos / sin tables [>= t_max][D / 2]
  const float* sn;
  h16_t* K;            // [B][Tmax][k_row]
  h16_t* V;
  h16_t* O;            // [B][H * D]
  float* ws;           // [B][H][S][D + 2]
  unsigned* cnt;       // [ceil(B / 16)][H], zero before the first call; left zero by every call
  long k_row, v_row, q_batch, k_batch, v_batch, o_batch;
  int B, S, H, t_max;
  float scale;
  const int* kv_lens;      // [B]
  const int* prefix_len;   // [1]
};

__device__ __forceinline__ void sh_unpack8(const uint4v& r, float* f) {
  f[0] = h16lo(r.x); f[1] = h16hi(r.x); f[2] = h16lo(r.y); f[3] = h16hi(r.y);
  f[4] = h16lo(r.z); f[5] = h16hi(r.z); f[6] = h16lo(r.w); f[7] = h16hi(r.w);
}

constexpr int SH_ROWS = 16;      // sequences per workgroup = columns of the MFMA B operand
constexpr int SH_MAXS = 32;      // key splits the merge tables in LDS hold

template <int D>
__global__ __launch_bounds__(256) void attn_decode_shared_kernel(SharedAttnArgs p) {
  constexpr int LPK = D / 8;            // lanes per key row (16 B each)
  constexpr int KPW = 64 / LPK;         // key rows a wave covers per load
  constexpr int KSTEPS = D / 32;        // MFMA k-steps over the head dim
  constexpr int DB = D / 16;            // 16-row blocks of O^T
  constexpr int SLD = D + 2;
  constexpr int NB = 4;                 // own phase: steps whose loads are issued together
  constexpr int VLD = D * 2 + 32;       // bytes per V row in the LDS tile: rows 8 dwords apart mod 64 banks (tr reads conflict-free)
  constexpr int SLOTS = D / 8;          // 16-B slots per key row
  constexpr int QS_BYTES = SH_ROWS * D * 2;
  constexpr int VT_BYTES = 32 * VLD;
  constexpr int ST_BYTES = SH_ROWS * SLD * 4;
  static_assert(ST_BYTES <= VT_BYTES, "a wave's prefix partial reuses its V tile");
  static_assert(2 * SH_ROWS * SH_MAXS * 4 <= 3 * QS_BYTES, "the merge tables reuse the q / k / v rows");
  __shared__ __attribute__((aligned(16))) char smem[3 * QS_BYTES + 4 * VT_BYTES + ST_BYTES];
  __shared__ unsigned arrival;
  h16_t* qs = reinterpret_cast<h16_t*>(smem);                    // [16][D] rotated q rows (16-bit)
  h16_t* kn = qs + SH_ROWS * D;                                  // [16][D] rotated new k rows
  h16_t* vn = kn + SH_ROWS * D;                                  // [16][D] new v rows
  char* vt_all = smem + 3 * QS_BYTES;                            // 4 wave-private V tiles; later the waves' prefix partials
  float* st_own = reinterpret_cast<float*>(vt_all + 4 * VT_BYTES);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPK, ks = lane / LPK;
  const int s = blockIdx.x, h = blockIdx.y, grp = blockIdx.z, S = p.S;
  const int b0 = grp * SH_ROWS;
  const int nrows = p.B - b0 < SH_ROWS ? p.B - b0 : SH_ROWS;
  int P = *p.prefix_len;
  P = P < 0 ? 0 : (P > p.t_max - 1 ? p.t_max - 1 : P);            // a bad value may give a wrong answer, never a fault
  const float sc2 = p.scale * 1.4426950408889634f;
  const size_t HD = (size_t)p.H * D;

  // ---- RoPE of the group's new q and k rows, cache append, rows to LDS: 16 lanes (D = 128) per row ----
  {
    const int r = wave * KPW + ks;
    if (r < SH_ROWS) {
      uint4v qr = {0u, 0u, 0u, 0u}, k_new = {0u, 0u, 0u, 0u}, v_new = {0u, 0u, 0u, 0u};
      if (r < nrows) {
        const size_t b = (size_t)(b0 + r);
        int pos = p.kv_lens[b];
        pos = pos < 0 ? 0 : (pos > p.t_max - 1 ? p.t_max - 1 : pos);
        const h16_t* row = p.qkv + b * p.q_batch;
        constexpr int HL = LPK / 2;
        const int v8 = (sub & (HL - 1)) * 8;
        const bool second = sub >= HL;
        const size_t own = (size_t)h * D + sub * 8, oth = (size_t)h * D + (sub ^ HL) * 8;
        float c[8], sn[8], a[8], bb[8], o[8];
        {
          const float4v c0 = *reinterpret_cast<const float4v*>(p.cs + (size_t)pos * (D / 2) + v8);
          const float4v c1 = *reinterpret_cast<const float4v*>(p.cs + (size_t)pos * (D / 2) + v8 + 4);
          const float4v s0 = *reinterpret_cast<const float4v*>(p.sn + (size_t)pos * (D / 2) + v8);
          const float4v s1 = *reinterpret_cast<const float4v*>(p.sn + (size_t)pos * (D / 2) + v8 + 4);
          c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w; c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w;
          sn[0] = s0.x; sn[1] = s0.y; sn[2] = s0.z; sn[3] = s0.w; sn[4] = s1.x; sn[5] = s1.y; sn[6] = s1.z; sn[7] = s1.w;
        }
        sh_unpack8(*reinterpret_cast<const uint4v*>(row + own), a);
        sh_unpack8(*reinterpret_cast<const uint4v*>(row + oth), bb);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = second ? __builtin_fmaf(a[e], c[e], bb[e] * sn[e]) : __builtin_fmaf(a[e], c[e], -(bb[e] * sn[e]));
        qr = {pack_h16x2(o[0], o[1]), pack_h16x2(o[2], o[3]), pack_h16x2(o[4], o[5]), pack_h16x2(o[6], o[7])};
        sh_unpack8(*reinterpret_cast<const uint4v*>(row + HD + own), a);
        sh_unpack8(*reinterpret_cast<const uint4v*>(row + HD + oth), bb);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = second ? __builtin_fmaf(a[e], c[e], bb[e] * sn[e]) : __builtin_fmaf(a[e], c[e], -(bb[e] * sn[e]));
        k_new = {pack_h16x2(o[0], o[1]), pack_h16x2(o[2], o[3]), pack_h16x2(o[4], o[5]), pack_h16x2(o[6], o[7])};
        v_new = *reinterpret_cast<const uint4v*>(row + 2 * HD + own);
        if (s == 0) {                                            // append the new row for the tokens to come
          *reinterpret_cast<uint4v*>(p.K + b * p.k_batch + (size_t)pos * p.k_row + own) = k_new;
          *reinterpret_cast<uint4v*>(p.V + b * p.v_batch + (size_t)pos * p.v_row + own) = v_new;
        }
      }
      *reinterpret_cast<uint4v*>(qs + r * D + sub * 8) = qr;      // rows past the batch: zero queries, discarded below
      *reinterpret_cast<uint4v*>(kn + r * D + sub * 8) = k_new;
      *reinterpret_cast<uint4v*>(vn + r * D + sub * 8) = v_new;
    }
  }
  __syncthreads();

  // ---- prefix phase: lane (g4 = lane / 16, qi = lane % 16) owns query column qi ----
  {
    const int g4 = lane >> 4, qi = lane & 15;
    char* vt = vt_all + wave * VT_BYTES;
    h16x8 qf[KSTEPS];
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk)
      qf[kk] = __builtin_bit_cast(h16x8, *reinterpret_cast<const uint4v*>(qs + qi * D + kk * 32 + g4 * 8));
    float4v oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) oacc[d] = {0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const h16_t* K0 = p.K + (size_t)h * D;                       // slot 0
    const h16_t* V0 = p.V + (size_t)h * D;
    // lane 4 q + pp of a 16-lane group supplies row q, columns 4 pp .. 4 pp + 3 of the [4 keys][16 d] block it reads transposed
    const int tr_off = (4 * g4 + (qi >> 2)) * VLD + (qi & 3) * 8;
    for (int t = s * 4 + wave; t * 32 < P; t += 4 * S) {         // wave-uniform trip count: EXEC stays full for the tr reads
      const int j0 = t * 32;
      uint4v kreg[2][KSTEPS], vreg[SLOTS / 2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        int key = j0 + 16 * c + qi;
        key = key < P ? key : P - 1;
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk)
          kreg[c][kk] = *reinterpret_cast<const uint4v*>(K0 + (size_t)key * p.k_row + kk * 32 + g4 * 8);
      }
#pragma unroll
      for (int it = 0; it < SLOTS / 2; ++it) {                   // 32 keys x SLOTS 16-B pieces over 64 lanes
        const int pk = it * 64 + lane;
        int key = j0 + pk / SLOTS;
        key = key < P ? key : P - 1;
        vreg[it] = *reinterpret_cast<const uint4v*>(V0 + (size_t)key * p.v_row + (pk % SLOTS) * 8);
      }
#pragma unroll
      for (int it = 0; it < SLOTS / 2; ++it) {
        const int pk = it * 64 + lane;
        *reinterpret_cast<uint4v*>(vt + (pk / SLOTS) * VLD + (pk % SLOTS) * 16) = vreg[it];
      }
      // S^T: sacc[c][r] = score of key j0 + 16 c + 4 g4 + r for query qi
      float4v sacc[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        sacc[c] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk)
          sacc[c] = G4R_MFMA_16X16X32(__builtin_bit_cast(h16x8, kreg[c][kk]), qf[kk], sacc[c], 0, 0, 0);
      }
      float mt = -INFINITY;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sv = sacc[c][r] * sc2;
          if (j0 + 16 * c + 4 * g4 + r >= P) sv = -INFINITY;
          sacc[c][r] = sv;
          mt = fmaxf(mt, sv);
        }
      mt = fmaxf(mt, __shfl_xor(mt, 16));
      mt = fmaxf(mt, __shfl_xor(mt, 32));                        // a tile holds at least one key < P: mt is finite
      const float m_new = fmaxf(m_run, mt);
      const float alpha = exp2f(m_run - m_new);                  // m_run = -inf -> 0
      float rs = 0.f;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = exp2f(sacc[c][r] - m_new);
          sacc[c][r] = e;
          rs += e;
        }
      l_run = l_run * alpha + rs;                                // this lane's share of the sum; the four shares meet at the end
      m_run = m_new;
      // B operand: k index 8 g4 + j  <->  key 4 g4 + j (j < 4), 16 + 4 g4 + j - 4 (j >= 4): what the two tr reads below deliver
      // p enters as a 16-bit value plus its 16-bit rounding residual (two MFMAs per V fragment), as in attention_cont.hip:
      // one rounding of p alone is the largest error term of such a kernel
      const uint4v pw = {pack_h16x2(sacc[0][0], sacc[0][1]), pack_h16x2(sacc[0][2], sacc[0][3]),
                         pack_h16x2(sacc[1][0], sacc[1][1]), pack_h16x2(sacc[1][2], sacc[1][3])};
      const uint4v pr = {pack_h16x2(sacc[0][0] - h16lo(pw.x), sacc[0][1] - h16hi(pw.x)),
                         pack_h16x2(sacc[0][2] - h16lo(pw.y), sacc[0][3] - h16hi(pw.y)),
                         pack_h16x2(sacc[1][0] - h16lo(pw.z), sacc[1][1] - h16hi(pw.z)),
                         pack_h16x2(sacc[1][2] - h16lo(pw.w), sacc[1][3] - h16hi(pw.w))};
      const h16x8 pf = __builtin_bit_cast(h16x8, pw), pf_lo = __builtin_bit_cast(h16x8, pr);
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const char* a = vt + tr_off + d * 32;
        const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(a));
        const short4v up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)(a + 16 * VLD));
        const short8 vv = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
#pragma unroll
        for (int r = 0; r < 4; ++r) oacc[d][r] *= alpha;
        oacc[d] = G4R_MFMA_16X16X32(__builtin_bit_cast(h16x8, vv), pf, oacc[d], 0, 0, 0);
        oacc[d] = G4R_MFMA_16X16X32(__builtin_bit_cast(h16x8, vv), pf_lo, oacc[d], 0, 0, 0);
      }
    }
    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
    // the wave's partial over its own V tile (its LDS accesses complete in order): O^T rows 16 d + 4 g4 + r, column qi
    float* stw = reinterpret_cast<float*>(vt);
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) stw[qi * SLD + d * 16 + 4 * g4 + r] = oacc[d][r];
    if (g4 == 0) { stw[qi * SLD + D] = m_run; stw[qi * SLD + D + 1] = l_run; }
  }

  // ---- own phase: the wave takes rows wave, wave + 4, ...; keys [P, len_b) of slot b and the new key ----
  for (int r = wave; r < nrows; r += 4) {
    const size_t b = (size_t)(b0 + r);
    int len = p.kv_lens[b];
    len = len < 0 ? 0 : (len > p.t_max - 1 ? p.t_max - 1 : len);
    const int Pc = P < len ? P : len;
    const int n = len - Pc + 1;                                  // own keys, the new one (j = n - 1) included
    int chunk = (n + S - 1) / S;
    chunk = (chunk + KPW - 1) / KPW * KPW;
    const int j_begin = s * chunk;
    const int j_end = j_begin + chunk < n ? j_begin + chunk : n;
    const h16_t* Kb = p.K + b * p.k_batch + (size_t)Pc * p.k_row + (size_t)h * D + sub * 8;
    const h16_t* Vb = p.V + b * p.v_batch + (size_t)Pc * p.v_row + (size_t)h * D + sub * 8;
    float q[8];
    sh_unpack8(*reinterpret_cast<const uint4v*>(qs + r * D + sub * 8), q);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] *= sc2;
    const uint4v k_new = *reinterpret_cast<const uint4v*>(kn + r * D + sub * 8);
    const uint4v v_new = *reinterpret_cast<const uint4v*>(vn + r * D + sub * 8);
    float m = -INFINITY, l = 0.f, o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j0 = j_begin; j0 < j_end; j0 += KPW * NB) {
      uint4v kv[NB], vv[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int j = j0 + u * KPW + ks;
        int jc = j < n - 1 ? j : n - 2;                          // never the row another workgroup is appending
        if (jc < 0) jc = 0;
        kv[u] = __builtin_nontemporal_load(reinterpret_cast<const uint4v*>(Kb + (size_t)jc * p.k_row));
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const uint4v*>(Vb + (size_t)jc * p.v_row));
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int j = j0 + u * KPW + ks;
        if (j == n - 1) { kv[u] = k_new; vv[u] = v_new; }          // the row being appended: from LDS
        float kf[8], vf[8];
        sh_unpack8(kv[u], kf);
        sh_unpack8(vv[u], vf);
        float sdot = q[0] * kf[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) sdot = fmaf(q[e], kf[e], sdot);
#pragma unroll
        for (int x = 1; x < LPK; x <<= 1) sdot += __shfl_xor(sdot, x);
        if (j < j_end) {
          const float mn = fmaxf(m, sdot);
          const float alpha = exp2f(m - mn), pj = exp2f(sdot - mn);
          l = l * alpha + pj;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = o[e] * alpha + pj * vf[e];
          m = mn;
        }
      }
    }
    // the KPW states of the wave meet by butterfly; group ks = 0 keeps the result
#pragma unroll
    for (int x = LPK; x < 64; x <<= 1) {
      const float mo = __shfl_xor(m, x), lo = __shfl_xor(l, x);
      const float mn = fmaxf(m, mo);
      const float wa = m == -INFINITY ? 0.f : exp2f(m - mn), wb = mo == -INFINITY ? 0.f : exp2f(mo - mn);
      l = l * wa + lo * wb;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float oo = __shfl_xor(o[e], x);
        o[e] = o[e] * wa + oo * wb;
      }
      m = mn;
    }
    if (ks == 0) {
      float* row = st_own + r * SLD;
#pragma unroll
      for (int e = 0; e < 8; ++e) row[sub * 8 + e] = o[e];
      if (sub == 0) { row[D] = m; row[D + 1] = l; }
    }
  }
  __syncthreads();

  // ---- one partial per (row, head, split): 4 prefix partials + the own partial ----
  float* part_ws = p.ws;
  for (int idx = tid; idx < SH_ROWS * D; idx += 256) {
    const int r = idx / D, d = idx % D;
    if (r >= nrows) continue;
    float mi[5], M = -INFINITY;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float* sti = i < 4 ? reinterpret_cast<const float*>(vt_all + i * VT_BYTES) : st_own;
      mi[i] = sti[r * SLD + D];
      M = fmaxf(M, mi[i]);
    }
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float* sti = i < 4 ? reinterpret_cast<const float*>(vt_all + i * VT_BYTES) : st_own;
      const float w = mi[i] == -INFINITY ? 0.f : exp2f(mi[i] - M);
      L += w * sti[r * SLD + D + 1];
      acc += w * sti[r * SLD + d];
    }
    const size_t b = (size_t)(b0 + r);
    if (S == 1) {
      p.O[b * p.o_batch + (size_t)h * D + d] = f32_to_h16(acc / L);
    } else {
      float* mine = part_ws + ((b * p.H + h) * S + s) * SLD;
      __hip_atomic_store(mine + d, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (d == 0) {
        __hip_atomic_store(mine + D, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + D + 1, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (S == 1) return;
  // ---- hand-off as in attn_decode_kernel: write-through stores, drained, then the arrival counter; the last workgroup of
  // this (group, head) reads the partials with agent-scope loads, writes the output rows and re-arms the counter ----
  unsigned* cnt = p.cnt + (size_t)grp * p.H + h;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) arrival = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (arrival != (unsigned)(S - 1)) return;
  float* wm = reinterpret_cast<float*>(smem);                    // [16][SH_MAXS] maxima, then sums
  float* wl = wm + SH_ROWS * SH_MAXS;
  for (int idx = tid; idx < SH_ROWS * S; idx += 256) {
    const int r = idx / S, i = idx % S;
    if (r >= nrows) continue;
    const float* part = part_ws + (((size_t)(b0 + r) * p.H + h) * S + i) * SLD;
    wm[r * SH_MAXS + i] = __hip_atomic_load(part + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    wl[r * SH_MAXS + i] = __hip_atomic_load(part + D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  for (int idx = tid; idx < SH_ROWS * D; idx += 256) {
    const int r = idx / D, d = idx % D;
    if (r >= nrows) continue;
    const size_t b = (size_t)(b0 + r);
    const float* part = part_ws + ((b * p.H + h) * S) * SLD;
    float mm = -INFINITY;
    for (int i = 0; i < S; ++i) mm = fmaxf(mm, wm[r * SH_MAXS + i]);
    float Lt = 0.f, a2 = 0.f;
    for (int i = 0; i < S; ++i) {
      const float m_i = wm[r * SH_MAXS + i];
      const float w = m_i == -INFINITY ? 0.f : exp2f(m_i - mm);
      Lt += w * wl[r * SH_MAXS + i];
      a2 += w * __hip_atomic_load(part + i * SLD + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    p.O[b * p.o_batch + (size_t)h * D + d] = f32_to_h16(a2 / Lt);
  }
  if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" {

// One decode step for `batch` sequences that share their first *prefix_len_dev cache rows (see the head of this file):
// the arguments of g4r_attn_decode_ragged_bf16 with a null rope_pos_dev, plus prefix_len_dev (int32 [1], device), the
// cache / table capacity `t_max` (rows per cache slot and rows of cos / sin: every length is clamped below it on the device,
// so a bad device value cannot fault), and the capacities of the workspace (floats) and the counters (uint32).
// workspace >= batch * H * splits * (head_dim + 2) floats, counters >= ceil(batch / 16) * H, zero before the first call.
// prefix_len_host / min_len_host / max_len_host: the prefix length and the smallest / largest kv length where the host
// knows them (negative: not known) -- a prefix longer than a sequence or a length beyond t_max is refused here.
int g4r_attn_decode_shared_bf16(const void* qkv, const float* cos_tab, const float* sin_tab, void* K, void* V, void* O,
                                float* workspace, long workspace_floats, unsigned* counters, long counters_len, int H,
                                int head_dim, long k_row, long v_row, float scale, int splits, const int* kv_lens_dev,
                                const int* prefix_len_dev, int batch, long q_batch, long k_batch, long v_batch,
                                long o_batch, int t_max, int prefix_len_host, int min_len_host, int max_len_host,
                                void* stream) {
  G4R_REQUIRE(H > 0 && batch >= 1 && t_max >= 1, "attn_decode_shared: bad shape");
  G4R_REQUIRE(head_dim == 64 || head_dim == 128, "attn_decode_shared: head_dim must be 64 or 128");
  G4R_REQUIRE(qkv && cos_tab && sin_tab && K && V && O && kv_lens_dev && prefix_len_dev, "attn_decode_shared: null pointer");
  G4R_REQUIRE(splits >= 1 && splits <= SH_MAXS, "attn_decode_shared: splits must be in [1, 32]");
  const long groups = (batch + SH_ROWS - 1) / SH_ROWS;
  G4R_REQUIRE(groups <= 65535 && H <= 65535, "attn_decode_shared: grid too large");
  G4R_REQUIRE(splits == 1 || (workspace && counters), "attn_decode_shared: split keys need workspace and counters");
  G4R_REQUIRE(splits == 1 || (workspace_floats >= (long)batch * H * splits * (head_dim + 2) && counters_len >= groups * H),
              "attn_decode_shared: workspace too small");
  G4R_REQUIRE(k_row % 8 == 0 && v_row % 8 == 0 && q_batch % 8 == 0 && k_batch % 8 == 0 && v_batch % 8 == 0 &&
                  o_batch % 8 == 0, "attn_decode_shared: strides must keep 16-byte alignment");
  G4R_REQUIRE(((uintptr_t)qkv | (uintptr_t)K | (uintptr_t)V | (uintptr_t)cos_tab | (uintptr_t)sin_tab) % 16 == 0,
              "attn_decode_shared: pointers must be 16-byte aligned");
  G4R_REQUIRE(k_row >= (long)H * head_dim && v_row >= (long)H * head_dim && q_batch >= 3L * H * head_dim &&
                  o_batch >= (long)H * head_dim, "attn_decode_shared: rows shorter than H * head_dim");
  G4R_REQUIRE(prefix_len_host < 0 || min_len_host < 0 || prefix_len_host <= min_len_host,
              "attn_decode_shared: the prefix is longer than a sequence");
  G4R_REQUIRE(prefix_len_host < t_max && min_len_host < t_max && max_len_host < t_max,
              "attn_decode_shared: lengths exceed the cache");
  SharedAttnArgs a = {(const h16_t*)qkv, cos_tab, sin_tab, (h16_t*)K, (h16_t*)V, (h16_t*)O, workspace, counters,
                      k_row, v_row, q_batch, k_batch, v_batch, o_batch, batch, splits, H, t_max, scale, kv_lens_dev,
                      prefix_len_dev};
  dim3 grid(splits, H, (unsigned)groups);
  if (head_dim == 64)
    hipLaunchKernelGGL((attn_decode_shared_kernel<64>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((attn_decode_shared_kernel<128>), grid, dim3(256), 0, (hipStream_t)stream, a);
  G4R_CHECK_LAUNCH("attn_decode_shared");
  return G4R_OK;
}

}  // extern "C"
