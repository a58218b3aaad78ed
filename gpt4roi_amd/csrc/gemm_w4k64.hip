// gemm_w4k64.hip -- the one-wave-per-SIMD kernel (gemm_bf16_w4k64_kernel) with its LDS-parked epilogues: tiles 34 / 36 of
// launch_gemm's switch (gemm_bf16.hip) when the launch does not take the persistent form (gemm_w4k64p.hip); tools build: tile 35.
#include "gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Epilogue of the one-wave-per-SIMD kernel (round 5): wave tile 128 x 128, FOUR waves.  In-kernel stamps of the first form
// (tools/wg_timeline.py, profiles/r05_wg_timeline.txt) put the K loop at 2221 cycles per 64 of K (MFMA floor 2048) and the
// shared epilogue above at 24.5 k cycles per tile -- 14 % of a K = 4096 tile: with half the waves of the ring kernel every
// wave runs twice the number of its serial read-back iterations (LDS read -> mode branches -> one store each).
// Here the mode is a TEMPLATE parameter of the kernel (the launcher picks it), so every instantiation carries one
// straight-line epilogue whose LDS reads and global accesses the compiler batches:
//   W4_P16  16-bit park, ONE pass (plain / bias / activation): the values are final BEFORE they are parked, so the wave parks
//           16-bit values (128 rows x 256 B) and reads them back as whole 16-byte runs of a row;
//   W4_SWIGLU  the (gate, up) column pairs sit in one lane: 64 outputs per row, parked as 16-bit;
//   W4_ROPE    the fused RoPE + KV-cache append of q|k|v: the projection is parked at the rounding point the unfused path had,
//              the wave's 128 columns are ONE head, so the rotation partner is column d +- 64 of the same parked row;
//   W4_WIDE    fp32 park, two passes of 64 rows (residual, fp32 output, K-slice partials): arithmetic after the park;
//   W4_GENERIC gemm_epilogue_lds (ragged N, unaligned rows).
// Same arithmetic and order as gemm_epilogue_lds (bias -> activation -> residual -> one rounding): bit-identical results.
// A wave whose 128 columns are not all inside N, or whose tile crosses row M, takes the guarded forms.
// ---------------------------------------------------------------------------------------------
#define G4R_W4_STAGGER_TICKS 0     // default start de-phasing step (10 ns ticks); see gemm_bf16_w4k64_kernel
struct W4Epi {
  static constexpr int RS16 = 256 + 16;         // 128 x 16-bit row + 16 B (rows stay 16-byte aligned for the b128 read-back)
  static constexpr int RSW = 128 + 16;          // SwiGLU: 64 x 16-bit outputs per row
  static constexpr int RS32 = 512 + 16;         // 128 x fp32 row + 16 B (EpiLds<4>::RS)
  static constexpr int WAVE_BYTES = 128 * RS16;  // >= 64 * RS32
};
static_assert(64 * W4Epi::RS32 <= W4Epi::WAVE_BYTES && 128 * W4Epi::RSW <= W4Epi::WAVE_BYTES && W4Epi::WAVE_BYTES >= EpiLds<4>::WAVE_BYTES,
              "every mode fits the wave's slice");

// read-back of a parked 16-bit tile: NR rows of RB bytes (LPR lanes x 16 B per row), whole rows of the output
template <int NR, int RS, int LPR, bool GUARD>
__device__ __forceinline__ void w4_copy_rows(const char* wave_lds, h16_t* dst0, long ldc, int lane, int rows_left) {
  constexpr int RPI = 64 / LPR;
  const int rrow = lane / LPR, rchunk = lane % LPR;
  const char* src = wave_lds + rrow * RS + rchunk * 16;
  h16_t* dst = dst0 + (long)rrow * ldc + rchunk * 8;
#pragma unroll
  for (int b = 0; b < NR / RPI; b += 8) {
    uint4v d[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) d[u] = *reinterpret_cast<const uint4v*>(src + (b + u) * RPI * RS);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (!GUARD || (b + u) * RPI + rrow < rows_left) *reinterpret_cast<uint4v*>(dst + (long)(b + u) * RPI * ldc) = d[u];
  }
}

template <int MODE, bool PROBE>
__device__ __forceinline__ void w4_epilogue(const GemmArgs& p, float16v (&acc)[4][4], char* wave_lds, int m_wave0, int n_wave0,
                                            int lane, int split, long long& park_t) {
  if (MODE == W4_GENERIC || n_wave0 + 128 > p.N) {         // (wave-uniform; W4_ROPE never sees a ragged tile: heads * 128 % 256 == 0)
    if (MODE != W4_ROPE) gemm_epilogue_lds<4, 4>(p, acc, wave_lds, m_wave0, n_wave0, lane, split);
    return;
  }
  if (m_wave0 >= p.M) return;                               // the whole wave tile is below the last row (wave-uniform)
  const int wr = lane & 31, wh = lane >> 5;
  const int rows_left = p.M - m_wave0;
  const bool full = rows_left >= 128;
  if (MODE == W4_SWIGLU) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float16v& c = acc[i][j];
          const float g0 = w4_acc(c, q * 4), u0 = w4_acc(c, q * 4 + 1), g1 = w4_acc(c, q * 4 + 2), u1 = w4_acc(c, q * 4 + 3);
          const float s0 = h16lo(pack_h16x2(g0 / (1.f + __expf(-g0)), 0.f));
          const float s1 = h16lo(pack_h16x2(g1 / (1.f + __expf(-g1)), 0.f));
          *reinterpret_cast<uint32_t*>(wave_lds + (i * 32 + wr) * W4Epi::RSW + (j * 16 + q * 4 + wh * 2) * 2) = pack_h16x2(s0 * u0, s1 * u1);
        }
    if (PROBE) park_t = __builtin_amdgcn_s_memtime();
    h16_t* dst0 = reinterpret_cast<h16_t*>(p.C) + (size_t)m_wave0 * p.ldc + (n_wave0 >> 1);
    if (full) w4_copy_rows<128, W4Epi::RSW, 8, false>(wave_lds, dst0, p.ldc, lane, rows_left);
    else w4_copy_rows<128, W4Epi::RSW, 8, true>(wave_lds, dst0, p.ldc, lane, rows_left);
    return;
  }
  if (MODE == W4_P16 || MODE == W4_ROPE) {
    // ---- 16-bit park: bias / activation applied in the accumulator layout (RoPE: the projection rounded as the unfused path did) ----
    const bool has_bias = MODE == W4_P16 && p.bias != nullptr;
    auto park16 = [&](auto act_tag) {                     // the activation is a compile-time constant of each copy
      constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float4v b = {0.f, 0.f, 0.f, 0.f};
          if (has_bias) b = *reinterpret_cast<const float4v*>(p.bias + n_wave0 + j * 32 + q * 8 + wh * 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float16v& c = acc[i][j];
            float v[4] = {w4_acc(c, q * 4) + b.x, w4_acc(c, q * 4 + 1) + b.y, w4_acc(c, q * 4 + 2) + b.z, w4_acc(c, q * 4 + 3) + b.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float x = v[k];
              v[k] = ACT == 0 ? x : (ACT == 1 ? fmaxf(x, 0.f) : (ACT == 2 ? x / (1.f + __expf(-1.702f * x)) : x / (1.f + __expf(-x))));
            }
            *reinterpret_cast<uint2v*>(wave_lds + (i * 32 + wr) * W4Epi::RS16 + (j * 32 + q * 8 + wh * 4) * 2) =
                uint2v{pack_h16x2(v[0], v[1]), pack_h16x2(v[2], v[3])};
          }
        }
    };
    const int act = MODE == W4_P16 ? p.act : 0;
    if (act == 0) park16(std::integral_constant<int, 0>{});
    else if (act == 1) park16(std::integral_constant<int, 1>{});
    else if (act == 2) park16(std::integral_constant<int, 2>{});
    else park16(std::integral_constant<int, 3>{});
    if (PROBE) park_t = __builtin_amdgcn_s_memtime();
    if (MODE == W4_P16) {
      h16_t* dst0 = reinterpret_cast<h16_t*>(p.C) + (size_t)m_wave0 * p.ldc + n_wave0;
      if (full) w4_copy_rows<128, W4Epi::RS16, 16, false>(wave_lds, dst0, p.ldc, lane, rows_left);
      else w4_copy_rows<128, W4Epi::RS16, 16, true>(wave_lds, dst0, p.ldc, lane, rows_left);
      return;
    }
    // fused RoPE + KV-cache append (gemm_epilogue_lds, act 5, states the arithmetic)
    const int rrow = lane >> 4, rchunk = lane & 15;      // 4 rows x 256 B per wave instruction
    const int part = n_wave0 / p.rope_HD;                // 0 q, 1 k, 2 v
    const int col0 = n_wave0 - part * p.rope_HD + rchunk * 8;
    const bool second = rchunk >= 8;
    const int d0 = (rchunk & 7) * 8;                     // position of this run inside its half of the head
#pragma unroll 4
    for (int it = 0; it < 32; ++it) {
      const int r = it * 4 + rrow;
      int m = m_wave0 + r;
      const bool live = m < p.M;
      if (!live) m = p.M - 1;                            // (reads stay in range; the store is masked)
      const uint4v own = *reinterpret_cast<const uint4v*>(wave_lds + r * W4Epi::RS16 + rchunk * 16);
      const uint4v mate = *reinterpret_cast<const uint4v*>(wave_lds + r * W4Epi::RS16 + (rchunk ^ 8) * 16);
      const int b = m / p.rope_T, t = m - b * p.rope_T;
      const int pos = p.rope_pos0 + t;
      uint4v o = own;
      if (part < 2) {
        const float* cp = p.rope_cos + (size_t)pos * 64 + d0;
        const float* sp = p.rope_sin + (size_t)pos * 64 + d0;
        const float4v c0 = *reinterpret_cast<const float4v*>(cp), c1 = *reinterpret_cast<const float4v*>(cp + 4);
        const float4v s0 = *reinterpret_cast<const float4v*>(sp), s1 = *reinterpret_cast<const float4v*>(sp + 4);
        const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const uint32_t ow[4] = {own.x, own.y, own.z, own.w}, mw[4] = {mate.x, mate.y, mate.z, mate.w};
        float v[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float a0 = h16lo(ow[k]), a1 = h16hi(ow[k]), b0 = h16lo(mw[k]), b1 = h16hi(mw[k]);
          v[2 * k] = second ? __builtin_fmaf(a0, cs[2 * k], b0 * sn[2 * k]) : __builtin_fmaf(a0, cs[2 * k], -(b0 * sn[2 * k]));
          v[2 * k + 1] = second ? __builtin_fmaf(a1, cs[2 * k + 1], b1 * sn[2 * k + 1])
                                : __builtin_fmaf(a1, cs[2 * k + 1], -(b1 * sn[2 * k + 1]));
        }
        o = uint4v{pack_h16x2(v[0], v[1]), pack_h16x2(v[2], v[3]), pack_h16x2(v[4], v[5]), pack_h16x2(v[6], v[7])};
      }
      h16_t* dst = part == 0 ? p.rope_q + (size_t)m * p.rope_HD + col0
                              : (part == 1 ? p.rope_k : p.rope_v) + (size_t)b * p.rope_kbatch + (size_t)pos * p.rope_krow + col0;
      if (live) *reinterpret_cast<uint4v*>(dst) = o;
    }
    return;
  }
  // ---- W4_WIDE: fp32 park, two passes of 64 rows: residual / fp32 output / K-slice partials ----
  const int rrow = lane >> 4, rcol = (lane & 15) * 8;
  float bias8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (p.bias != nullptr && p.splits == 1) {
    const float4v b0 = *reinterpret_cast<const float4v*>(p.bias + n_wave0 + rcol), b1 = *reinterpret_cast<const float4v*>(p.bias + n_wave0 + rcol + 4);
    bias8[0] = b0.x; bias8[1] = b0.y; bias8[2] = b0.z; bias8[3] = b0.w; bias8[4] = b1.x; bias8[5] = b1.y; bias8[6] = b1.z; bias8[7] = b1.w;
  }
  const int n = n_wave0 + rcol;
  auto readback = [&](int mh, auto act_tag) {
    constexpr int ACT = decltype(act_tag)::value;        // -1: K-slice partials
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int r = it * 4 + rrow;
      int m = mh + r;
      const bool live = m < p.M;
      if (!live) m = p.M - 1;                            // (reads stay in range; the stores are masked)
      const float4v a0 = *reinterpret_cast<const float4v*>(wave_lds + r * W4Epi::RS32 + rcol * 4);
      const float4v a1 = *reinterpret_cast<const float4v*>(wave_lds + r * W4Epi::RS32 + rcol * 4 + 16);
      if (ACT < 0) {
        float* dst = p.ws + ((size_t)split * p.M + m) * p.N + n;
        if (live) {
          *reinterpret_cast<float4v*>(dst) = a0;
          *reinterpret_cast<float4v*>(dst + 4) = a1;
        }
        continue;
      }
      float v[8] = {a0.x + bias8[0], a0.y + bias8[1], a0.z + bias8[2], a0.w + bias8[3],
                    a1.x + bias8[4], a1.y + bias8[5], a1.z + bias8[6], a1.w + bias8[7]};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float x = v[k];
        v[k] = ACT <= 0 ? x : (ACT == 1 ? fmaxf(x, 0.f) : (ACT == 2 ? x / (1.f + __expf(-1.702f * x)) : x / (1.f + __expf(-x))));
      }
      if (p.residual) {
        const uint4v rr = *reinterpret_cast<const uint4v*>(p.residual + (size_t)m * p.ldr + n);
        v[0] += h16lo(rr.x); v[1] += h16hi(rr.x); v[2] += h16lo(rr.y); v[3] += h16hi(rr.y);
        v[4] += h16lo(rr.z); v[5] += h16hi(rr.z); v[6] += h16lo(rr.w); v[7] += h16hi(rr.w);
      }
      if (p.out_f32) {
        float* dst = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
        if (live) {
          *reinterpret_cast<float4v*>(dst) = float4v{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<float4v*>(dst + 4) = float4v{v[4], v[5], v[6], v[7]};
        }
      } else if (live) {
        *reinterpret_cast<uint4v*>(reinterpret_cast<h16_t*>(p.C) + (size_t)m * p.ldc + n) =
            uint4v{pack_h16x2(v[0], v[1]), pack_h16x2(v[2], v[3]), pack_h16x2(v[4], v[5]), pack_h16x2(v[6], v[7])};
      }
    }
  };
  const int act = p.splits > 1 ? -1 : p.act;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float16v& c = acc[half * 2 + i2][j];
          *reinterpret_cast<float4v*>(wave_lds + (i2 * 32 + wr) * W4Epi::RS32 + (j * 32 + q * 8 + wh * 4) * 4) =
              float4v{c[q * 4], c[q * 4 + 1], c[q * 4 + 2], c[q * 4 + 3]};       // (ds_write_b128 takes its data straight from AGPRs)
        }
    if (PROBE && half == 0) park_t = __builtin_amdgcn_s_memtime();
    const int mh = m_wave0 + half * 64;
    if (act < 0) readback(mh, std::integral_constant<int, -1>{});
    else if (act == 0) readback(mh, std::integral_constant<int, 0>{});
    else if (act == 1) readback(mh, std::integral_constant<int, 1>{});
    else if (act == 2) readback(mh, std::integral_constant<int, 2>{});
    else readback(mh, std::integral_constant<int, 3>{});
  }
}

// ---------------------------------------------------------------------------------------------
// Round 5 -- one-wave-per-SIMD kernel, second form ("w4k64", tile_cfg 34): 256 x 256 tile, FOUR waves (2 x 2), wave tile
// 128 x 128 (16 accumulators of 32x32 = all 256 AGPRs), K tiles of 64 in TWO LDS buffers that are refilled as soon as they
// are consumed.
// Why (profiles/r05_vendor_ab.txt): a same-process A/B showed the vendor library at 1550 TF/s SUSTAINED on random operands
// where the ring ping-pong kernel above does 1160-1235 -- the "power-cap ceiling" of round 4 was a ceiling of THAT kernel.
// Its 8 waves x (128 x 64) read 192 KB of fragments per CU per 64 of K; 4 waves x (128 x 128) read 128 KB for the same
// flops, every fragment read and every LDS-DMA piece can be hidden under the OWN wave's MFMAs (one wave per SIMD: 7 free
// issue slots per 32-cycle MFMA), and there are two workgroup barriers per 64 MFMAs instead of four hand-offs.
// Layout: a K tile is rows of 128 B (64 elements); a 1 KiB LDS-DMA piece = 8 rows x 128 B = WHOLE cache lines; the 16-byte
// slot of k-chunk c of row r sits at slot c ^ ((r >> 1) & 7) (source-side swizzle, conflict-free for the lane groups of
// ds_read_b128, MI355X_MICROARCH.md LDS table).  Per K tile a wave issues 8 + 8 pieces and 16 + 16 fragment reads.
// Schedule of tile i (buffer X = i & 1; H0 / H1 = the fragments of k-steps 0,1 / 2,3, 64 + 64 VGPRs):
//   A: 20 MFMA on H0           | 16 reads H1 <- X                                   | lgkmcnt(0), barrier  (X is consumed)
//   B: 24 MFMA on H0 / H1      | 12 pieces of tile i+2 -> X                         | vmcnt(12), barrier   (tile i+1 landed)
//   C: 20 MFMA on H1           | 16 reads H0 <- X^1 (tile i+1), last 4 pieces       |
// so a tile's pieces have 1.3 tiles (~2700 cycles) to land.  AMODE 1 / 2 (implicit-GEMM convolution): the tap shift goes
// into the per-lane offset, an out-of-image tap is an offset beyond the descriptor's extent (zeros), K tile = 64 channels
// of one tap.
// ---------------------------------------------------------------------------------------------
template <int AMODE, bool PROBE, int EPI, bool MI16P = false>
__global__ __launch_bounds__(256, 1) void gemm_bf16_w4k64_kernel(GemmArgs p) {
  constexpr int BM = 256, BN = 256, NW = 4, BKT = 64, ROWB = 128, NP = 8;
  constexpr int TM = 4, TN = 4;
  constexpr int A_BYTES = BM * ROWB, STAGE_BYTES = (BM + BN) * ROWB;      // 32 KB + 32 KB per K tile
  extern __shared__ __attribute__((aligned(16))) char smem[];            // 2 * STAGE_BYTES = 128 KB
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nwg = p.tiles_m * p.tiles_n;
  int wg, split;
  g4r_workgroup_tile_slice(nwg, false, wg, split);
  int tile_m, tile_n;
  g4r_tile_coords(wg, p.tiles_m, p.tiles_n, p.n_fastest, p.group_m, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int t_begin = split * p.tiles_per_split;
  int t_end = t_begin + p.tiles_per_split;
  const int nt_total = p.K / BKT;
  if (t_end > nt_total) t_end = nt_total;
  // PROBE (tools/wg_timeline.py, tile 35): wave 0 of every workgroup records entry / loop begin / loop end / exit (s_memtime),
  // its XCC id and the 100 MHz wall clock at ws + 16 + 8 * blockIdx.x (int64) -- the convention of the ring kernel's probe
  long long* wg_stamps = reinterpret_cast<long long*>(p.ws) + 16 + 8 * (long)blockIdx.x;
  const bool wg_probe = PROBE && blockIdx.y == 0 && wave == 0;       // (wave-uniform: all 64 lanes store the same stamp)
  if (PROBE) { if (wg_probe) { wg_stamps[0] = __builtin_amdgcn_s_memtime(); wg_stamps[4] = __builtin_amdgcn_s_getreg(6164); wg_stamps[5] = wall_clock64(); } }

  // De-phasing (round 5): every workgroup of a launch runs the same number of K tiles, so all 256 CUs reach their epilogue at
  // the same moment and the 32 MB of a wave's outputs hit the memory system as ONE burst while every matrix pipe idles.  The
  // first 256 workgroups (one per CU) start `phase x stagger_ticks x 10 ns` late, phase = 0..7 by CU slot inside the XCD; later
  // workgroups inherit the phase of the CU they land on, so at any moment only ~1/8 of the CUs are storing.
  if (p.stagger_ticks > 0) {
    const int lin = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    const int phase = (lin >> 3) & 7;
    if (lin < 256 && phase != 0) {
      const long long t_go = wall_clock64() + (long long)phase * p.stagger_ticks;
      while (wall_clock64() < t_go) __builtin_amdgcn_s_sleep(8);
    }
  }

  // piece j of this wave covers rows 8 * (4 j + wave) + lane / 8; lane % 8 is the 16-byte slot it writes
  int a_voff[NP], b_voff[NP];
  unsigned a_ok[NP];
  int a_pitch[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int row = (j * NW + wave) * 8 + (lane >> 3);
    const int kslot = (lane & 7) ^ ((row >> 1) & 7);
    int gm = m0 + row;
    if (gm > p.M - 1) gm = p.M - 1;
    a_voff[j] = (gm * p.lda + kslot * 8) * 2;
    int gn = n0 + row;
    if (gn > p.N - 1) gn = p.N - 1;
    b_voff[j] = (gn * p.ldw + kslot * 8) * 2;
    a_ok[j] = 0;
    a_pitch[j] = p.Wd * p.lda;
    if (AMODE >= 1) {
      int h = p.H, w = p.Wd, local = gm;
      if (AMODE == 2) {
        int lv = 0;
#pragma unroll
        for (int q = 1; q < 4; ++q)
          if (q < p.n_lvl && gm >= p.lvl_start[q]) lv = q;
        h = p.lvl_h[lv]; w = p.lvl_w[lv];
        local = gm - p.lvl_start[lv];
        a_pitch[j] = w * p.lda;
      }
      const int hw = h * w;
      const int rem = local - (local / hw) * hw;
      const int y = rem / w, x = rem - y * w;
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int yy = y + tp / 3 - 1, xx = x + tp % 3 - 1;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) a_ok[j] |= 1u << tp;
      }
    }
  }
  // the NEXT K tile to stage (tiles are staged strictly in order): dense = a K offset; conv = (64-channel slice, group, tap),
  // taps fastest, walked by a counter
  int st_t = t_begin, st_ct = 0, st_g = 0, st_tap = 0;
  if (AMODE >= 1) {
    const int n_taps = 9 * p.groups;
    st_ct = t_begin / n_taps;
    const int rem = t_begin - st_ct * n_taps;
    st_g = rem / 9;
    st_tap = rem - st_g * 9;
  }
  struct TileSrc { int a_soff, w_soff, tap, dy, dx; };
  auto next_tile = [&]() {
    TileSrc ts;
    ts.tap = ts.dy = ts.dx = 0;
    ts.a_soff = ts.w_soff = st_t * BKT * 2;
    ++st_t;
    if (AMODE >= 1) {
      const int c0 = st_ct * BKT;
      ts.tap = st_tap;
      ts.dy = st_tap / 3 - 1;
      ts.dx = st_tap - (st_tap / 3) * 3 - 1;
      ts.a_soff = (int)(((long)st_g * p.a_group_stride + c0) * 2);
      ts.w_soff = ((st_g * 9 + st_tap) * p.Cin + c0) * 2;
      if (++st_tap == 9) {
        st_tap = 0;
        if (++st_g == p.groups) { st_g = 0; ++st_ct; }
      }
    }
    return ts;
  };
  // piece q of a K tile for this wave: q < 8 -> rows of A, else rows of W
  auto piece = [&](int q, const TileSrc& ts, int buf) {
    char* sa = smem + buf * STAGE_BYTES;
    if (q < NP) {
      int voff = a_voff[q];
      if (AMODE == 1) voff += (ts.dy * p.Wd + ts.dx) * p.lda * 2;
      if (AMODE == 2) voff += (ts.dy * a_pitch[q] + ts.dx * p.lda) * 2;
      if (AMODE >= 1 && !((a_ok[q] >> ts.tap) & 1u)) voff = (int)0x80000000;      // beyond num_records: reads as zeros
      g4r_buffer_piece(p.A, p.a_bytes, sa + (q * NW + wave) * 1024, voff, ts.a_soff);
    } else {
      g4r_buffer_piece(p.W, p.w_bytes, sa + A_BYTES + ((q - NP) * NW + wave) * 1024, b_voff[q - NP], ts.w_soff);
    }
  };
  float16v acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int frow = lane & 31, fsw = (frow >> 1) & 7, fhi = lane >> 5;
  const int a_row_off = (wm * 128 + frow) * ROWB;
  const int b_row_off = A_BYTES + (wn * 128 + frow) * ROWB;
  h16x8 fa[4][TM], fw[4][TN];                  // [k-step][block]: k-steps 0,1 = H0, 2,3 = H1
  auto ldfrag = [&](auto ks_tag, int buf) {
    constexpr int ks = decltype(ks_tag)::value;
    const char* sb = smem + buf * STAGE_BYTES;
    const int slot = ((2 * ks + fhi) ^ fsw) << 4;
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[ks][i] = *reinterpret_cast<const h16x8*>(sb + a_row_off + i * 32 * ROWB + slot);
#pragma unroll
    for (int j = 0; j < TN; ++j) fw[ks][j] = *reinterpret_cast<const h16x8*>(sb + b_row_off + j * 32 * ROWB + slot);
  };
  // MI16P (tools build, debug mode 65; results are WRONG by construction): the same loads, fragment reads and barriers, but every
  // 32 x 32 x 16 product is replaced by TWO v_mfma_f32_16x16x32 on four-register accumulators -- the same FLOPs per K tile through
  // the other MFMA shape, to measure what that shape buys under the power cap with the real kernel's traffic around it
  float4v acc4[MI16P ? TM : 1][MI16P ? TN : 1][4];
  if (MI16P) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc4[MI16P ? i : 0][MI16P ? j : 0][r] = float4v{0.f, 0.f, 0.f, 0.f};
  }
  auto mma_rows = [&](auto ks_tag, auto i0_tag, auto i1_tag) {    // rows [i0, i1) of k-step ks
    constexpr int ks = decltype(ks_tag)::value, i0 = decltype(i0_tag)::value, i1 = decltype(i1_tag)::value;
#pragma unroll
    for (int i = i0; i < i1; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (MI16P) {
          constexpr int r0 = 2 * (ks & 1);
          acc4[i][j][r0] = G4R_MFMA_16X16X32(fw[ks][j], fa[ks][i], acc4[i][j][r0], 0, 0, 0);
          acc4[i][j][r0 + 1] = G4R_MFMA_16X16X32(fa[ks][i], fw[ks][j], acc4[i][j][r0 + 1], 0, 0, 0);
        } else {
          acc[i][j] = G4R_MFMA_32X32X16(fw[ks][j], fa[ks][i], acc[i][j], 0, 0, 0);
        }
      }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using I4 = std::integral_constant<int, 4>;

  const int nt = t_end - t_begin;
  if (nt > 0) {
    {
      const TileSrc ts = next_tile();
#pragma unroll
      for (int q = 0; q < 2 * NP; ++q) piece(q, ts, 0);
    }
    if (nt > 1) {
      const TileSrc ts = next_tile();
#pragma unroll
      for (int q = 0; q < 2 * NP; ++q) piece(q, ts, 1);
      __builtin_amdgcn_s_waitcnt(0x4f70);                     // vmcnt(16): tile 0 has landed
    } else {
      __builtin_amdgcn_s_waitcnt(0x0f70);                     // vmcnt(0)
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    ldfrag(I0{}, 0);
    ldfrag(I1{}, 0);
    // sched_group_barrier masks (LLVM SchedGroupMask): 0x8 MFMA, 0x10 VMEM, 0x100 DS read
    auto body = [&](int i, auto steady_tag) {
      constexpr bool STEADY = decltype(steady_tag)::value;      // tiles i+1, i+2 exist: no branches in the body
      const int buf = i & 1;
      // ---- A: k-step 0 + the first row of k-step 1 | H1 <- X, one read per MFMA ----
      ldfrag(I2{}, buf);
      ldfrag(I3{}, buf);
      mma_rows(I0{}, I0{}, I4{});
      mma_rows(I1{}, I0{}, I1{});
#pragma unroll
      for (int n = 0; n < 16; ++n) {
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xc07f);                      // lgkmcnt(0): every fragment of X is in registers (the builtin,
      asm volatile("" ::: "memory");                           //   not inline asm: the compiler's counter model sees it)
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();                            // ... in every wave: X may be overwritten
      __builtin_amdgcn_sched_barrier(0);
      // ---- B: rest of k-step 1 + three rows of k-step 2 | pieces 0-11 of tile i+2 -> X, one per two MFMAs ----
      TileSrc ts2 = {};
      const bool more = STEADY || i + 2 < nt;
      if (more) {
        ts2 = next_tile();
#pragma unroll
        for (int q = 0; q < 12; ++q) piece(q, ts2, buf);
      }
      mma_rows(I1{}, I1{}, I4{});
      mma_rows(I2{}, I0{}, I3{});
      if (STEADY) {
#pragma unroll
        for (int n = 0; n < 12; ++n) {
          __builtin_amdgcn_sched_group_barrier(0x8, 2, 1);
          __builtin_amdgcn_sched_group_barrier(0x10, 1, 1);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) __builtin_amdgcn_s_waitcnt(0x0f7c);            // vmcnt(12): tile i+1 has landed (only this tile's 12 in flight)
      else __builtin_amdgcn_s_waitcnt(0x0f70);                 // vmcnt(0)
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---- C: last row of k-step 2 + k-step 3 | H0 <- X^1 (tile i+1), one read per MFMA; the last 4 pieces ----
      if (STEADY || i + 1 < nt) {
        ldfrag(I0{}, buf ^ 1);
        ldfrag(I1{}, buf ^ 1);
      }
      if (more) {
#pragma unroll
        for (int q = 12; q < 16; ++q) piece(q, ts2, buf);
      }
      mma_rows(I2{}, I3{}, I4{});
      mma_rows(I3{}, I0{}, I4{});
      if (STEADY) {
#pragma unroll
        for (int n = 0; n < 16; ++n) {
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 2);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 2);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 2);
          __builtin_amdgcn_sched_group_barrier(0x10, 1, 2);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    if (PROBE) { if (wg_probe) wg_stamps[1] = __builtin_amdgcn_s_memtime(); }
    int i = 0;
    for (; i + 2 < nt; ++i) body(i, std::true_type{});
    for (; i < nt; ++i) body(i, std::false_type{});
    if (PROBE) { if (wg_probe) wg_stamps[2] = __builtin_amdgcn_s_memtime(); }
  }
  if (MI16P) {       // no epilogue: the accumulators only have to stay alive (C is left untouched)
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += acc4[MI16P ? i : 0][MI16P ? j : 0][r >> 2][r & 3];
    if (sum == 12345.678f) reinterpret_cast<float*>(p.C)[lane] = sum;
    return;
  }
  __syncthreads();   // the operand buffers are idle: stage the epilogue through them
  long long park_t = 0;
  w4_epilogue<EPI, PROBE>(p, acc, smem + wave * W4Epi::WAVE_BYTES, m0 + wm * 128, n0 + wn * 128, lane, split, park_t);
  if (PROBE) { if (wg_probe) { wg_stamps[3] = __builtin_amdgcn_s_memtime(); wg_stamps[6] = wall_clock64(); wg_stamps[7] = park_t; } }
}

template <int AMODE, bool PROBE, int EPI, bool MI16P = false>
int launch_w4k64_epi(GemmArgs& p, hipStream_t stream) {
  const size_t ring = 2 * (256 + 256) * 64 * 2, epi = 4 * (size_t)W4Epi::WAVE_BYTES;
  const size_t lds = ring > epi ? ring : epi;
  auto kern = gemm_bf16_w4k64_kernel<AMODE, PROBE, EPI, MI16P>;
  static G4rPerDeviceOnce attr_set;
  if (int rc = gemm_raise_lds_limit(attr_set, reinterpret_cast<const void*>(kern), lds, "gemm_w4k64: hipFuncSetAttribute")) return rc;
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n, p.splits), dim3(256), lds, stream, p);
  G4R_CHECK_LAUNCH("gemm_bf16_w4k64");
  return G4R_OK;
}

}  // namespace

G4R_GEMM_NS_OPEN

template <int AMODE, bool PROBE>
int launch_w4k64(GemmArgs& p, hipStream_t stream) {
  {
    // extents for the buffer descriptors: the last byte a clamped row / in-image tap can touch
    size_t ab = (size_t)p.M * p.lda * 2, wb = (size_t)p.N * p.ldw * 2;
    if (AMODE == 1) ab = ((size_t)(p.groups - 1) * p.a_group_stride + (size_t)p.M * p.lda) * 2;
    // operands of 2 GiB and more do not fit a buffer descriptor's 32-bit extent: the ring ping-pong tile with plain
    // global_load_lds pieces (64-bit addresses) serves them, as it did before this kernel became the default (e.g. the
    // stage-2 data gradient dgu[tokens, 22016] x W^T above ~48.7 k tokens)
    if (ab >= 0x7fffffffu || wb >= 0x7fffffffu) {
      if (PROBE) return g4r_note_error(G4R_ERR_UNSUPPORTED, "gemm_w4k64 (probe): operands of 2 GiB and more");
      return launch_pp32<AMODE, false, 256, 256, false, (AMODE >= 1 ? 1 : 0)>(p, stream);
    }
    p.a_bytes = (unsigned)ab;
    p.w_bytes = (unsigned)wb;
  }
  if (p.K % 64 != 0 || (AMODE >= 1 && p.Cin % 64 != 0)) return g4r_note_error(G4R_ERR_INVALID_ARG, "gemm_w4k64: K (Cin) must be a multiple of 64");
  gemm_split_geometry(p, 64);
  p.tiles_m = g4r_ceil_div(p.M, 256);
  p.tiles_n = g4r_ceil_div(p.N, 256);
  // start de-phasing of launches of several waves of tiles (tools: debug modes 70 + n = n x 0.25 us per phase, 79 = off)
  p.stagger_ticks = 0;
  if ((long)p.tiles_m * p.tiles_n * p.splits > 2 * 256) p.stagger_ticks = G4R_W4_STAGGER_TICKS;
  if (g_gemm_dbg >= 70 && g_gemm_dbg < 79) p.stagger_ticks = (g_gemm_dbg - 70) * 25;
  if (g_gemm_dbg == 79) p.stagger_ticks = 0;
  // the epilogue mode (W4Epi): the straight-line forms need 16-byte rows on every operand they touch
  const bool wide = p.splits > 1 || p.out_f32 || p.residual != nullptr;
  int mode = W4_GENERIC;
  if ((p.N & 7) == 0) {
    if (p.act == 5) mode = W4_ROPE;
    else if (p.splits > 1) mode = W4_WIDE;
    else if ((p.ldc & 7) == 0 && (p.residual == nullptr || (p.ldr & 7) == 0) && (p.act != 4 || ((p.ldc & 7) == 0 && !wide)))
      mode = wide ? W4_WIDE : (p.act == 4 ? W4_SWIGLU : W4_P16);
  }
  if (p.act == 5 && mode != W4_ROPE) return g4r_note_error(G4R_ERR_INVALID_ARG, "gemm_w4k64: the fused RoPE epilogue needs N % 8 == 0");
  // Round 6: launches of more than one wave of tiles take the PERSISTENT form (gemm_bf16_w4k64p_kernel: one workgroup per CU
  // walks the tiles, the next tile's first K tiles land during the epilogue, which stores straight from the accumulators).
  // tools: debug mode 61 = off (A/B arm; the bit-identity tests compare the two forms).
  if (!PROBE && g_gemm_dbg != 61 && p.splits == 1 && (p.N % 256) == 0 && !p.out_f32 && (p.ldc & 7) == 0) {
    const int ncu = g4r_cu_count();
    const long tiles = (long)p.tiles_m * p.tiles_n;
    const bool mode_ok = mode == W4_P16 || mode == W4_SWIGLU || mode == W4_ROPE || (mode == W4_WIDE && p.residual != nullptr);
    size_t cb = (size_t)p.M * p.ldc * 2, rb = p.residual ? (size_t)p.M * p.ldr * 2 : 0, rq = 0, rkv = 0;
    if (mode == W4_ROPE) {
      const long nb = p.M / p.rope_T;
      rq = (size_t)p.M * p.rope_HD * 2;
      rkv = (size_t)((nb - 1) * p.rope_kbatch + (long)(p.rope_pos0 + p.rope_T - 1) * p.rope_krow + p.rope_HD) * 2;
      cb = rq;
    }
    // (K < 2048 -- the ViT block GEMMs -- stays per tile: with 16 K tiles per output tile the epilogue is a fifth of a tile and the
    //  per-tile form hides its store drain behind the next workgroup's start: 6-9 % faster there, profiles/r06_persist_ab.jsonl)
    if (mode_ok && tiles > ncu && (p.K >= 2048 || p.persist_any_k) && p.M < (1 << 20) && cb < 0x7fffffffu && rb < 0x7fffffffu && rq < 0x7fffffffu && rkv < 0x7fffffffu) {
      p.c_bytes = (unsigned)cb; p.r_bytes = (unsigned)rb; p.rq_bytes = (unsigned)rq; p.rkv_bytes = (unsigned)rkv;
      if (AMODE != 0) {
        // The convolution over all pyramid levels has a persistent form too (LEAN addressing, see the kernel: every level starts on a
        // tile boundary -- true for the pyramids of the path at any batch: 64 P^2, 16 P^2 and 4 P^2 rows per image are multiples of
        // 256 at P = 16 and 24).  It is bit-identical to the per-tile form and 4-6 % SLOWER (1282 vs 1358 TF/s at batch 16,
        // profiles/r06_conv_persist_ab.txt: with 144 K tiles per output tile the boundary is 5 % of a tile and hipcc spills around it),
        // so it is compiled into the tools build only (debug mode 63, tools/conv_persist_ab.py).
#ifdef G4R_TOOLS_BUILD
        if constexpr (AMODE == 2) {
          bool aligned = p.groups == 1;
          for (int l = 1; l < p.n_lvl; ++l) aligned = aligned && (p.lvl_start[l] % 256) == 0;
          if (g_gemm_dbg == 63 && aligned && mode == W4_P16 && p.bias == nullptr && p.act <= 1) return launch_w4k64p_epi<2, W4_P16>(p, ncu, stream);
        }
#endif
      } else {
        switch (mode) {
          case W4_P16: return launch_w4k64p_epi<0, W4_P16>(p, ncu, stream);
          case W4_SWIGLU: return launch_w4k64p_epi<0, W4_SWIGLU>(p, ncu, stream);
          case W4_ROPE: return launch_w4k64p_epi<0, W4_ROPE>(p, ncu, stream);
          default: return launch_w4k64p_epi<0, W4_WIDE>(p, ncu, stream);
        }
      }
    }
  }
#ifdef G4R_TOOLS_BUILD
  if (AMODE == 0 && !PROBE && g_gemm_dbg == 65 && mode == W4_P16) return launch_w4k64_epi<0, false, W4_P16, true>(p, stream);   // MFMA-shape probe
#endif
  int rc = G4R_OK;
  if (AMODE != 0) {                       // the convolutions: bias / ReLU only
    rc = (mode == W4_P16) ? launch_w4k64_epi<AMODE, false, W4_P16>(p, stream)
                          : (mode == W4_WIDE ? launch_w4k64_epi<AMODE, false, W4_WIDE>(p, stream) : launch_w4k64_epi<AMODE, false, W4_GENERIC>(p, stream));
  } else if (PROBE) {
    rc = mode == W4_P16 ? launch_w4k64_epi<0, PROBE, W4_P16>(p, stream) : launch_w4k64_epi<0, PROBE, W4_WIDE>(p, stream);
  } else {
    switch (mode) {
      case W4_P16: rc = launch_w4k64_epi<0, false, W4_P16>(p, stream); break;
      case W4_SWIGLU: rc = launch_w4k64_epi<0, false, W4_SWIGLU>(p, stream); break;
      case W4_ROPE: rc = launch_w4k64_epi<0, false, W4_ROPE>(p, stream); break;
      case W4_WIDE: rc = launch_w4k64_epi<0, false, W4_WIDE>(p, stream); break;
      default: rc = launch_w4k64_epi<0, false, W4_GENERIC>(p, stream); break;
    }
  }
  return rc != G4R_OK ? rc : gemm_reduce_tail(p, stream);
}

template int launch_w4k64<0, false>(GemmArgs&, hipStream_t);
template int launch_w4k64<1, false>(GemmArgs&, hipStream_t);
template int launch_w4k64<2, false>(GemmArgs&, hipStream_t);
#ifdef G4R_TOOLS_BUILD
template int launch_w4k64<0, true>(GemmArgs&, hipStream_t);    // tile 35
#endif

}  // namespace G4R_GEMM_NS
