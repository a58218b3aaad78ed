// gemm_w4k64p.hip -- the persistent form of the one-wave-per-SIMD kernel (gemm_bf16_w4k64p_kernel): what launch_w4k64
// (gemm_w4k64.hip) picks for tiles 34 / 36 on launches of more than one wave of tiles.
#include <atomic>

#include "gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Round 6 -- the PERSISTENT form of the one-wave-per-SIMD kernel ("w4k64p"): the same 256 x 256 tile, K loop and schedule as
// gemm_bf16_w4k64_kernel, but ONE workgroup per CU walks the launch's tiles (tile t of CU slot b is the t-th tile the
// hardware dispatcher would have handed that slot: linear id b + 256 t through the same XCD map), and the epilogue goes
// straight from the accumulator registers to memory.
// Why (profiles/r05_wg_timeline.txt): of a K = 4096 tile's lifetime the K loop is 0.88; the rest is the
// prologue (~3 k cycles: nothing to multiply until the first two K tiles have landed), the LDS-parked epilogue (~16 k) and
// the gap between a workgroup's exit and its successor's start (the launch of 9 waves of tiles takes ~5 us per wave longer
// than 9 workgroup lifetimes).  Here the first two K tiles of the NEXT tile are requested (LDS-DMA into the idle operand
// buffers) before the epilogue of the finished one starts, so they land while it stores; nothing is parked in LDS:
//   * in the swapped-operand accumulator layout a lane holds, of output row m, the column quads {8 q + 4 wh .. + 3}.  After
//     rounding to 16 bit a quad is two dwords; ONE v_permlane32_swap per dword between the quads q = 2 p of the upper
//     half-wave and q = 2 p + 1 of the lower one leaves every lane with 8 CONSECUTIVE columns = one 16-byte store (lane
//     wh = 0: columns 16 p .. + 7, wh = 1: 16 p + 8 .. + 15), so a store instruction writes 32 contiguous bytes of 32 rows:
//     4 096 line requests per tile against 32 768 for the 8-byte direct epilogue of round 1 and ~1 000 + two LDS passes for
//     the parked one;
//   * stores are buffer stores: a row beyond M gets an offset beyond the descriptor's extent (dropped by the hardware), so
//     the number of vector-memory instructions of an epilogue is a compile-time constant and the wait for the next tile's
//     first K tile can be COUNTED (vmcnt = 16 pieces of its second K tile + the epilogue's stores) instead of draining the
//     store queue -- vector-memory operations retire in issue order on gfx9 (loads and stores share vmcnt);
//   * SwiGLU (two levels of the swap), the fused RoPE + KV-cache append (the rotation partner d +- 64 is accumulator
//     [i][j +- 2] of the SAME lane and register: no exchange at all) and bias / activation / residual are done in the
//     accumulator layout with the arithmetic and rounding points of w4_epilogue: bit-identical results.
// Serves launches of more than one wave of tiles with N % 256 == 0, no K slices and 16-bit outputs; everything else stays on
// gemm_bf16_w4k64_kernel (launch_w4k64).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t w4p_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// two quads of 16-bit values (x = quad 2 p, y = quad 2 p + 1; two dwords each) -> this lane's 8 consecutive columns
__device__ __forceinline__ uint4v w4p_gather8(uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1) {
  const auto ra = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
  const auto rb = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
  return uint4v{ra[0], rb[0], ra[1], rb[1]};
}

constexpr int w4p_stores(int epi) { return epi == W4_SWIGLU ? 16 : 32; }     // buffer stores per wave and tile

// Epilogue of the persistent form, phase 1: accumulators -> final 16-bit values (bias / activation / residual / SwiGLU / RoPE in
// the accumulator layout, the arithmetic and rounding points of w4_epilogue), transposed 32 rows at a time through the wave's
// 8 KB of spare LDS into ROW-major 16-byte chunks: chunk (lane % LPR) of row 32 i + RPI u + lane / LPR of the wave tile (LPR = 16
// lanes per 256-byte row, RPI = 4 rows per instruction; SwiGLU: 8 and 8) goes back into the accumulator registers of pass i,
// which are dead by then -- acc[i][u / 4][4 (u % 4) .. + 3] -- so the finished tile waits for its stores in AGPRs and costs no
// VGPRs while the next tile's offsets are computed and its pieces issued.
// Every ordinary load and every LDS operation of the epilogue happens HERE, i.e. before the next tile's LDS-DMA pieces are
// issued: an LDS instruction behind a wave's own pieces waits until they have landed, and hipcc waits vmcnt(0) for an ordinary
// load next to an LDS-DMA in flight.  A parked row is 32 (SwiGLU: 16) slots of 8 B; slot s of row r sits at s ^ (r & 15): the
// 16 lanes of a ds_write_b64 group (16 rows, one slot) hit 16 different slots, the 16 lanes of a ds_read_b128 group (one row) 16
// different chunks.
template <int EPI, bool LIGHT = false>      // LIGHT (the convolutions): no bias, activation none / ReLU only -- two copies instead of eight
__device__ __forceinline__ void w4p_epilogue_compute(const GemmArgs& p, float16v (&acc)[4][4], char* wave_lds, int m_wave0, int n_wave0,
                                                     int lane) {
  const int wr = lane & 31, wh = lane >> 5;
  constexpr int OOR = (int)0x80000000;                    // beyond any extent: a load returns zeros
  constexpr int RB = EPI == W4_SWIGLU ? 128 : 256;        // parked row bytes
  constexpr int LPR = RB / 16, RPI = 64 / LPR, NU = 32 / RPI;
  const int rrow = lane / LPR, rch = lane % LPR;
  auto read_back = [&](int i) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int r = u * RPI + rrow;
      // 16-byte chunk rch of row r = slots 2 rch, 2 rch + 1 -> chunk rch ^ ((r & 15) >> 1), halves swapped when r is odd
      uint4v v = *reinterpret_cast<const uint4v*>(wave_lds + r * RB + ((rch ^ ((r & 15) >> 1)) << 4));
      if (r & 1) v = uint4v{v.z, v.w, v.x, v.y};
      float16v& dst = acc[i][u >> 2];
      dst[(u & 3) * 4 + 0] = __uint_as_float(v.x);
      dst[(u & 3) * 4 + 1] = __uint_as_float(v.y);
      dst[(u & 3) * 4 + 2] = __uint_as_float(v.z);
      dst[(u & 3) * 4 + 3] = __uint_as_float(v.w);
    }
  };
  if (EPI == W4_SWIGLU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float16v& c = acc[i][j];
        uint32_t d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float g0 = w4_acc(c, q * 4), u0 = w4_acc(c, q * 4 + 1), g1 = w4_acc(c, q * 4 + 2), u1 = w4_acc(c, q * 4 + 3);
          const float s0 = h16lo(pack_h16x2(g0 / (1.f + __expf(-g0)), 0.f));
          const float s1 = h16lo(pack_h16x2(g1 / (1.f + __expf(-g1)), 0.f));
          d[q] = pack_h16x2(s0 * u0, s1 * u1);             // output columns 16 j + 4 q + 2 wh + {0, 1}
        }
        // quads q = 0,1 -> the 8-byte slot 4 j + wh of this row (4 consecutive outputs); q = 2,3 -> slot 4 j + 2 + wh
        const auto c0 = __builtin_amdgcn_permlane32_swap(d[0], d[1], false, false);
        const auto c1 = __builtin_amdgcn_permlane32_swap(d[2], d[3], false, false);
        *reinterpret_cast<uint2v*>(wave_lds + wr * RB + (((4 * j + wh) ^ (wr & 15)) << 3)) = uint2v{c0[0], c0[1]};
        *reinterpret_cast<uint2v*>(wave_lds + wr * RB + (((4 * j + 2 + wh) ^ (wr & 15)) << 3)) = uint2v{c1[0], c1[1]};
      }
      read_back(i);
    }
    return;
  }
  if (EPI == W4_ROPE) {
    // d = 32 jj + 8 q + 4 wh + k (< 64) is accumulator block jj, its rotation partner d + 64 block jj + 2, SAME lane and register
    const int part = n_wave0 / p.rope_HD;                // 0 q, 1 k, 2 v (wave-uniform; the wave's 128 columns are one head)
    const float inv_T = 1.0f / (float)p.rope_T;          // (m + 0.5) / T never lands within 0.5 / T of an integer: exact for M < 2^20
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (part < 2) {
        int m = m_wave0 + i * 32 + wr;
        if (m > p.M - 1) m = p.M - 1;                    // (table reads stay in range; the row is not stored)
        const int b = (int)(((float)m + 0.5f) * inv_T);
        const int tab = (p.rope_pos0 + m - b * p.rope_T) * 64 + wh * 4;
        float4v cs[8], sn[8];                            // this pass's table entries, all in flight together
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          cs[e] = *reinterpret_cast<const float4v*>(p.rope_cos + tab + e * 8);
          sn[e] = *reinterpret_cast<const float4v*>(p.rope_sin + tab + e * 8);
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4v c_ = cs[jj * 4 + q], s_ = sn[jj * 4 + q];
            const float c4[4] = {c_.x, c_.y, c_.z, c_.w}, s4[4] = {s_.x, s_.y, s_.z, s_.w};
            float lo[4], hi[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              // the unfused path stored the projection in 16 bit before rotating it: keep that rounding point
              const float a = h16lo(pack_h16x2(w4_acc(acc[i][jj], q * 4 + k), 0.f));
              const float bb = h16lo(pack_h16x2(w4_acc(acc[i][jj + 2], q * 4 + k), 0.f));
              lo[k] = __builtin_fmaf(a, c4[k], -(bb * s4[k]));      // rotate_half: a' = a cos - b sin
              hi[k] = __builtin_fmaf(bb, c4[k], a * s4[k]);         //              b' = b cos + a sin
            }
            *reinterpret_cast<uint2v*>(wave_lds + wr * RB + (((8 * jj + 2 * q + wh) ^ (wr & 15)) << 3)) =
                uint2v{pack_h16x2(lo[0], lo[1]), pack_h16x2(lo[2], lo[3])};
            *reinterpret_cast<uint2v*>(wave_lds + wr * RB + (((8 * (jj + 2) + 2 * q + wh) ^ (wr & 15)) << 3)) =
                uint2v{pack_h16x2(hi[0], hi[1]), pack_h16x2(hi[2], hi[3])};
          }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float16v& c = acc[i][j];
            *reinterpret_cast<uint2v*>(wave_lds + wr * RB + (((8 * j + 2 * q + wh) ^ (wr & 15)) << 3)) =
                uint2v{pack_h16x2(w4_acc(c, q * 4), w4_acc(c, q * 4 + 1)), pack_h16x2(w4_acc(c, q * 4 + 2), w4_acc(c, q * 4 + 3))};
          }
      }
      read_back(i);
    }
    return;
  }
  // ---- W4_P16 (bias -> activation -> one rounding) and W4_WIDE (... -> + residual -> one rounding): 16-bit output ----
  const bool has_res = EPI == W4_WIDE && p.residual != nullptr;
  const __amdgpu_buffer_rsrc_t rr = w4p_rsrc(has_res ? (const void*)p.residual : (const void*)p.C, has_res ? p.r_bytes : 0u);
  const bool has_bias = p.bias != nullptr;
  auto run = [&](auto act_tag, auto bias_tag) {           // activation and bias are compile-time constants of each copy:
    constexpr int ACT = decltype(act_tag)::value;         // straight-line code (a branch per quad costs more than the quad)
    constexpr bool BIAS = decltype(bias_tag)::value;
    // The residual tile is loaded ROW-major -- 32 loads of 4 rows x 256 B per wave tile, all in flight together (128 VGPRs: the
    // operand fragments are dead) -- and transposed into the accumulator layout through the same 8 KB of LDS, one 32-row pass
    // ahead of the values it is added to.  (Loading it in the accumulator layout -- 8 B per lane on 32 different rows per
    // instruction -- took ~400 cycles per load instruction: profiles/r06_w4p_timeline.txt.)
    uint4v resrow[EPI == W4_WIDE ? 32 : 1];
    if (EPI == W4_WIDE) {
#pragma unroll
      for (int e = 0; e < 32; ++e) {
        const int m = m_wave0 + (e >> 3) * 32 + (e & 7) * 4 + rrow;
        const int roff = (m < p.M && has_res) ? (m * p.ldr + n_wave0 + rch * 8) * 2 : OOR;          // (absent / beyond M: zeros)
        resrow[e] = __builtin_amdgcn_raw_buffer_load_b128(rr, roff, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint2v res[16];                                     // this lane's residual quads of pass i (slot 8 j + 2 q + wh of row wr)
      if (EPI == W4_WIDE) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {                     // row-major chunk -> the parked-row layout (see read_back)
          const int r = u * 4 + rrow;
          uint4v v = resrow[i * 8 + u];
          if (r & 1) v = uint4v{v.z, v.w, v.x, v.y};
          *reinterpret_cast<uint4v*>(wave_lds + r * RB + ((rch ^ ((r & 15) >> 1)) << 4)) = v;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e)
          res[e] = *reinterpret_cast<const uint2v*>(wave_lds + wr * RB + (((2 * e + wh) ^ (wr & 15)) << 3));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float16v& c = acc[i][j];
          // (+ 0.f: the per-tile form always adds its bias quad, zeros when absent -- keeps -0 -> +0 bit-identical)
          float v[4] = {w4_acc(c, q * 4) + 0.f, w4_acc(c, q * 4 + 1) + 0.f, w4_acc(c, q * 4 + 2) + 0.f, w4_acc(c, q * 4 + 3) + 0.f};
          if (BIAS) {
            const float4v b = *reinterpret_cast<const float4v*>(p.bias + n_wave0 + j * 32 + q * 8 + wh * 4);
            v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float x = v[k];
            v[k] = ACT == 0 ? x : (ACT == 1 ? fmaxf(x, 0.f) : (ACT == 2 ? x / (1.f + __expf(-1.702f * x)) : x / (1.f + __expf(-x))));
          }
          if (EPI == W4_WIDE) {
            const uint2v r0 = res[j * 4 + q];
            v[0] += h16lo(r0.x); v[1] += h16hi(r0.x); v[2] += h16lo(r0.y); v[3] += h16hi(r0.y);
          }
          // columns 32 j + 8 q + 4 wh .. + 3 = slot 8 j + 2 q + wh of the row
          *reinterpret_cast<uint2v*>(wave_lds + wr * RB + (((8 * j + 2 * q + wh) ^ (wr & 15)) << 3)) =
              uint2v{pack_h16x2(v[0], v[1]), pack_h16x2(v[2], v[3])};
        }
      read_back(i);
    }
  };
  if (LIGHT) {
    if (p.act == 0) run(std::integral_constant<int, 0>{}, std::false_type{});
    else run(std::integral_constant<int, 1>{}, std::false_type{});
  } else if (has_bias) {
    if (p.act == 0) run(std::integral_constant<int, 0>{}, std::true_type{});
    else if (p.act == 1) run(std::integral_constant<int, 1>{}, std::true_type{});
    else if (p.act == 2) run(std::integral_constant<int, 2>{}, std::true_type{});
    else run(std::integral_constant<int, 3>{}, std::true_type{});
  } else {
    if (p.act == 0) run(std::integral_constant<int, 0>{}, std::false_type{});
    else if (p.act == 1) run(std::integral_constant<int, 1>{}, std::false_type{});
    else if (p.act == 2) run(std::integral_constant<int, 2>{}, std::false_type{});
    else run(std::integral_constant<int, 3>{}, std::false_type{});
  }
}

// Phase 2: the 32 (SwiGLU: 16) whole-row buffer stores of a wave tile.  A row beyond M gets an offset beyond the descriptor's
// extent (dropped by the hardware), so the count is a compile-time constant.
template <int EPI>
__device__ __forceinline__ void w4p_epilogue_store(const GemmArgs& p, float16v (&acc)[4][4], int m_wave0, int n_wave0, int lane) {
  constexpr int OOR = (int)0x80000000;
  constexpr int LPR = EPI == W4_SWIGLU ? 8 : 16, RPI = 64 / LPR, NU = 32 / RPI;
  static_assert(4 * NU == w4p_stores(EPI), "the persistent kernel's counted vmcnt waits assume this many stores");
  const int rrow = lane / LPR, rch = lane % LPR;
  auto chunk = [&](int i, int u) {
    const float16v& c = acc[i][u >> 2];
    return uint4v{__float_as_uint(w4_acc(c, (u & 3) * 4)), __float_as_uint(w4_acc(c, (u & 3) * 4 + 1)),
                  __float_as_uint(w4_acc(c, (u & 3) * 4 + 2)), __float_as_uint(w4_acc(c, (u & 3) * 4 + 3))};
  };
  if (EPI == W4_ROPE) {
    const int part = n_wave0 / p.rope_HD;
    const int col0 = n_wave0 - part * p.rope_HD + rch * 8;
    const __amdgpu_buffer_rsrc_t rc = part == 0 ? w4p_rsrc(p.rope_q, p.rq_bytes) : w4p_rsrc(part == 1 ? p.rope_k : p.rope_v, p.rkv_bytes);
    const float inv_T = 1.0f / (float)p.rope_T;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int m = m_wave0 + i * 32 + u * RPI + rrow;
        const int b = (int)(((float)m + 0.5f) * inv_T);
        const int pos = p.rope_pos0 + m - b * p.rope_T;
        const long o = part == 0 ? (long)m * p.rope_HD + col0 : (long)b * p.rope_kbatch + (long)pos * p.rope_krow + col0;
        __builtin_amdgcn_raw_buffer_store_b128(chunk(i, u), rc, m < p.M ? (int)(o * 2) : OOR, 0, 0);
      }
    return;
  }
  const __amdgpu_buffer_rsrc_t rc = w4p_rsrc(p.C, p.c_bytes);
  const int ncol = (EPI == W4_SWIGLU ? (n_wave0 >> 1) : n_wave0) + rch * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int m = m_wave0 + i * 32 + u * RPI + rrow;
      __builtin_amdgcn_raw_buffer_store_b128(chunk(i, u), rc, m < p.M ? (m * p.ldc + ncol) * 2 : OOR, 0, 0);
    }
}

template <int AMODE, int EPI>
__global__ __launch_bounds__(256, 1) void gemm_bf16_w4k64p_kernel(GemmArgs p) {
  constexpr int BM = 256, BN = 256, NW = 4, BKT = 64, ROWB = 128, NP = 8;
  constexpr int TM = 4, TN = 4;
  constexpr int A_BYTES = BM * ROWB, STAGE_BYTES = (BM + BN) * ROWB;      // 32 KB + 32 KB per K tile
  extern __shared__ __attribute__((aligned(16))) char smem[];            // 2 * STAGE_BYTES = 128 KB + 4 x 8 KB of epilogue staging
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int total = p.tiles_m * p.tiles_n;                                // (no K slices in this form)
  const int nt = p.K / BKT;

  // per-lane piece state.  Dense: one byte offset per piece (rows clamped at M - 1 / N - 1).  AMODE 2 (the convolution over all
  // pyramid levels, LEAN form): the launcher guarantees that every level starts on a tile boundary, so a tile lies in ONE level
  // (map size and row pitch are wave-uniform) and the rows of piece j are the rows of piece 0 + 32 j: ONE offset for A and one for
  // W (the 32 j rows go into the instruction's scalar offset), the tap masks of the 8 piece rows, and no clamping (a row beyond M
  // is beyond the descriptor's extent: zeros) -- 10 registers instead of 32, which is what lets this form fit beside the 128
  // fragment registers without moving an accumulator block to VGPRs.
  constexpr bool LEAN = AMODE == 2;
  int a_voff[LEAN ? 1 : NP], b_voff[LEAN ? 1 : NP];
  unsigned a_ok[NP];
  int a_pitch[LEAN ? 1 : NP];
  int lean_pitch = 0;                         // LEAN: bytes between map rows of the tile's level (wave-uniform)
  int m0 = 0, n0 = 0;
  // work item -> tile, and the per-lane piece offsets of that tile (piece j of this wave covers rows 8 (4 j + wave) + lane / 8;
  // lane % 8 is the 16-byte slot it writes: gemm_bf16_w4k64_kernel)
  auto setup = [&](int item) {
    const int q = total >> 3, r = total & 7, xcd = item & 7, idx = item >> 3;     // g4r_workgroup_tile_slice on a linear id
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    int tile_m, tile_n;
    g4r_tile_coords(wg, p.tiles_m, p.tiles_n, p.n_fastest, p.group_m, tile_m, tile_n);
    m0 = tile_m * BM;
    n0 = tile_n * BN;
    // (opaque copy of the lane id: without it hipcc hoists the tile-invariant parts of the offsets out of the persistent loop
    //  and keeps them alive through the K loop, where the convolution forms then spill)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    if constexpr (LEAN) {
      int lv = 0;
#pragma unroll
      for (int q2 = 1; q2 < 4; ++q2)
        if (q2 < p.n_lvl && m0 >= p.lvl_start[q2]) lv = q2;                 // (scalar: the tile's level)
      const int h = p.lvl_h[lv], w = p.lvl_w[lv], hw = h * w;
      lean_pitch = w * p.lda * 2;
      const float inv_hw = 1.0f / (float)hw, inv_w = 1.0f / (float)w;       // (x + 0.5) / d is never within 0.5 / d of an integer: exact below 2^22
      const int row0 = wave * 8 + (ln >> 3);
      const int kslot = (ln & 7) ^ ((row0 >> 1) & 7);                       // (the same for all 8 pieces: (32 j) >> 1 is a multiple of 8)
      a_voff[0] = ((m0 + row0) * p.lda + kslot * 8) * 2;
      b_voff[0] = ((n0 + row0) * p.ldw + kslot * 8) * 2;
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int gm = m0 + row0 + j * 32;
        const int local = gm - p.lvl_start[lv];
        const int img = (int)(((float)local + 0.5f) * inv_hw);
        const int rem = local - img * hw;
        const int y = (int)(((float)rem + 0.5f) * inv_w), x = rem - y * w;
        unsigned ok = 0;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
          const int yy = y + tp / 3 - 1, xx = x + tp % 3 - 1;
          if (yy >= 0 && yy < h && xx >= 0 && xx < w) ok |= 1u << tp;
        }
        a_ok[j] = gm < p.M ? ok : 0u;                                       // (rows beyond M: every tap reads zeros)
      }
    } else {
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int row = (j * NW + wave) * 8 + (ln >> 3);
        const int kslot = (ln & 7) ^ ((row >> 1) & 7);
        int gm = m0 + row;
        if (gm > p.M - 1) gm = p.M - 1;
        a_voff[j] = (gm * p.lda + kslot * 8) * 2;
        int gn = n0 + row;
        if (gn > p.N - 1) gn = p.N - 1;
        b_voff[j] = (gn * p.ldw + kslot * 8) * 2;
        a_ok[j] = 0;
        a_pitch[j] = p.Wd * p.lda;
        if (AMODE >= 1) {
          const int h = p.H, w = p.Wd, local = gm;
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
    }
  };
  // the NEXT K tile to stage (tiles are staged strictly in order): dense = a K offset; conv = (64-channel slice, group, tap),
  // taps fastest, walked by a counter
  int st_t = 0, st_ct = 0, st_g = 0, st_tap = 0;
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
  auto piece = [&](int q, const TileSrc& ts, int buf) {
    char* sa = smem + buf * STAGE_BYTES;
    if constexpr (LEAN) {
      if (q < NP) {
        // the tap shift and the 32 q rows of piece q are wave-uniform (one level per tile): ONE scalar added to the lane's base
        // offset.  (They cannot ride in the instruction's scalar offset: the descriptor's range check sees the VECTOR offset alone,
        // and base + a negative tap shift is "out of range" before the scalar offset brings it back -- zeros instead of texels.)
        int voff = a_voff[0] + (q * 32 * p.lda * 2 + ts.dy * lean_pitch + ts.dx * p.lda * 2);
        if (!((a_ok[q] >> ts.tap) & 1u)) voff = (int)0x80000000;            // beyond num_records: reads as zeros
        g4r_buffer_piece(p.A, p.a_bytes, sa + (q * NW + wave) * 1024, voff, ts.a_soff);
      } else {
        g4r_buffer_piece(p.W, p.w_bytes, sa + A_BYTES + ((q - NP) * NW + wave) * 1024, b_voff[0], ts.w_soff + (q - NP) * 32 * p.ldw * 2);
      }
      return;
    }
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
  // the first two K tiles of the tile `setup` prepared: 16 + 16 pieces into buffers 0 / 1
  auto prologue = [&]() {
    st_t = st_ct = st_g = st_tap = 0;
    {
      const TileSrc ts = next_tile();
#pragma unroll
      for (int q = 0; q < 2 * NP; ++q) piece(q, ts, 0);
    }
    if (nt > 1) {
      const TileSrc ts = next_tile();
#pragma unroll
      for (int q = 0; q < 2 * NP; ++q) piece(q, ts, 1);
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
  auto mma_rows = [&](auto ks_tag, auto i0_tag, auto i1_tag, auto zero_tag) {    // rows [i0, i1) of k-step ks
    constexpr int ks = decltype(ks_tag)::value, i0 = decltype(i0_tag)::value, i1 = decltype(i1_tag)::value;
    constexpr bool ZERO = decltype(zero_tag)::value;              // the first products of an output tile: C = 0 (an inline constant)
    const float16v z16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = i0; i < i1; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = G4R_MFMA_32X32X16(fw[ks][j], fa[ks][i], ZERO ? z16 : acc[i][j], 0, 0, 0);
  };
  using NoZ = std::false_type;
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using I4 = std::integral_constant<int, 4>;
  // the K-tile body of gemm_bf16_w4k64_kernel (phases A / B / C, see there), unchanged
  // RELAX: the epilogue's stores of the previous output tile sit between K tile 1's pieces and K tile 2's in the (in-order)
  // vector-memory queue; the wait for K tile 1 at the end of phase B of K tile 0 may leave them in flight (RELAX = their
  // number), which gives them two K tiles (~4.4 k cycles) to drain behind the matrix pipe instead of one phase
  auto body = [&](int i, auto steady_tag, auto relax_tag) {
    constexpr bool STEADY = decltype(steady_tag)::value;      // tiles i+1, i+2 exist: no branches in the body
    constexpr int RELAX = decltype(relax_tag)::value;
    const int buf = i & 1;
    ldfrag(I2{}, buf);
    ldfrag(I3{}, buf);
    mma_rows(I0{}, I0{}, I4{}, NoZ{});      // (C = 0 for the first K tile after an epilogue instead of zeroing the accumulators
                                            //  was tried: hipcc then spills 50-200 VGPRs in every epilogue mode)
    mma_rows(I1{}, I0{}, I1{}, NoZ{});
#pragma unroll
    for (int n = 0; n < 16; ++n) {
      __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xc07f);                      // lgkmcnt(0): every fragment of X is in registers
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();                            // ... in every wave: X may be overwritten
    __builtin_amdgcn_sched_barrier(0);
    TileSrc ts2 = {};
    const bool more = STEADY || i + 2 < nt;
    if (more) {
      ts2 = next_tile();
#pragma unroll
      for (int q = 0; q < 12; ++q) piece(q, ts2, buf);
    }
    mma_rows(I1{}, I1{}, I4{}, NoZ{});
    mma_rows(I2{}, I0{}, I3{}, NoZ{});
    if (STEADY) {
#pragma unroll
      for (int n = 0; n < 12; ++n) {
        __builtin_amdgcn_sched_group_barrier(0x8, 2, 1);
        __builtin_amdgcn_sched_group_barrier(0x10, 1, 1);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
      if (RELAX == 32) __builtin_amdgcn_s_waitcnt(0x8f7c);   // vmcnt(44): tile i+1 has landed; 32 stores + this tile's 12 pieces may be in flight
      else if (RELAX == 16) __builtin_amdgcn_s_waitcnt(0x4f7c);   // vmcnt(28)
      else __builtin_amdgcn_s_waitcnt(0x0f7c);               // vmcnt(12): tile i+1 has landed (and every older store has retired)
    } else {
      __builtin_amdgcn_s_waitcnt(0x0f70);                    // vmcnt(0)
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (STEADY || i + 1 < nt) {
      ldfrag(I0{}, buf ^ 1);
      ldfrag(I1{}, buf ^ 1);
    }
    if (more) {
#pragma unroll
      for (int q = 12; q < 16; ++q) piece(q, ts2, buf);
    }
    mma_rows(I2{}, I3{}, I4{}, NoZ{});
    mma_rows(I3{}, I0{}, I4{}, NoZ{});
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

  // Order at a tile boundary: epilogue phase 1 (every load and LDS operation of the epilogue; results in registers) -> the next
  // tile's offsets and its first two K tiles' pieces -> epilogue phase 2 (the stores).  The pieces land while the stores issue,
  // and the wait for them below leaves the stores in flight.  (The epilogue sits at the loop's END: with it at the head hipcc
  // moves all 256 accumulators to VGPRs and spills.)
  int item = blockIdx.x;
  setup(item);
  prologue();
  // vector-memory operations issued AFTER the first K tile's 16 pieces when the loop is entered: the second K tile's 16
  // pieces and, when the epilogue ran behind the pieces, its stores (a compile-time count: a row beyond M is a dropped
  // store, not a skipped one).  They retire in issue order (loads and stores share vmcnt on gfx9), so at most that many
  // outstanding = the first K tile has landed.
  int behind = nt > 1 ? 16 : 0;
#ifdef G4R_W4P_PROBE
  // tools/w4p_timeline.py (build with G4R_EXTRA_HIPCC_FLAGS=-DG4R_W4P_PROBE, pass a workspace): wave 0 of every workgroup records
  // s_memtime at [tile top, K loop begin, K loop end, epilogue end] of each of its tiles at ws + (blockIdx.x * 16 + tile) * 4
  long long* stamps = reinterpret_cast<long long*>(p.ws) + (long)blockIdx.x * 64;
  int tile_no = 0;
#define G4R_W4P_STAMP(slot) do { if (p.ws != nullptr && wave == 0 && tile_no < 16) stamps[tile_no * 4 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define G4R_W4P_STAMP(slot) do { } while (0)
#endif
  for (;;) {
    G4R_W4P_STAMP(0);
    if (behind >= 48) __builtin_amdgcn_s_waitcnt(0xcf70);        // vmcnt(48)
    else if (behind >= 32) __builtin_amdgcn_s_waitcnt(0x8f70);   // vmcnt(32)
    else if (behind >= 16) __builtin_amdgcn_s_waitcnt(0x4f70);   // vmcnt(16)
    else __builtin_amdgcn_s_waitcnt(0x0f70);                     // vmcnt(0)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    ldfrag(I0{}, 0);
    ldfrag(I1{}, 0);
    G4R_W4P_STAMP(1);
    int i = 0;
    if (behind > 16 && nt > 2) {                                 // (behind > 16: an epilogue's stores are in the queue)
      body(0, std::true_type{}, std::integral_constant<int, w4p_stores(EPI)>{});
      i = 1;
    }
    for (; i + 2 < nt; ++i) body(i, std::true_type{}, I0{});
    for (; i < nt; ++i) body(i, std::false_type{}, I0{});
    // every wave has read its last fragments (phase A of the last K tile ends in a barrier) and no piece is in flight: the
    // operand buffers are idle
    G4R_W4P_STAMP(2);
    const int em = m0 + wm * 128, en = n0 + wn * 128;
    const int next = item + (int)gridDim.x;
    const bool has_next = next < total;
    w4p_epilogue_compute<EPI, (AMODE != 0)>(p, acc, smem + 2 * STAGE_BYTES + wave * 8192, em, en, lane);
    if (has_next) {
      setup(next);
      prologue();
    }
    w4p_epilogue_store<EPI>(p, acc, em, en, lane);
    G4R_W4P_STAMP(3);
#ifdef G4R_W4P_PROBE
    ++tile_no;
#endif
    if (!has_next) break;
#pragma unroll
    for (int i2 = 0; i2 < TM; ++i2)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i2][j][r] = 0.f;
    behind = (nt > 1 ? 16 : 0) + w4p_stores(EPI);
    item = next;
  }
}

}  // namespace

G4R_GEMM_NS_OPEN

template <int AMODE, int EPI>
int launch_w4k64p_epi(GemmArgs& p, int grid, hipStream_t stream) {
  const size_t lds = 2 * (256 + 256) * 64 * 2 + 4 * 8192;        // the operand ring + 8 KB of epilogue staging per wave = all 160 KB
  auto kern = gemm_bf16_w4k64p_kernel<AMODE, EPI>;
  static G4rPerDeviceOnce attr_set;
  if (int rc = gemm_raise_lds_limit(attr_set, reinterpret_cast<const void*>(kern), lds, "gemm_w4k64p: hipFuncSetAttribute")) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, p);
  G4R_CHECK_LAUNCH("gemm_bf16_w4k64p");
  return G4R_OK;
}

template int launch_w4k64p_epi<0, W4_P16>(GemmArgs&, int, hipStream_t);
template int launch_w4k64p_epi<0, W4_SWIGLU>(GemmArgs&, int, hipStream_t);
template int launch_w4k64p_epi<0, W4_ROPE>(GemmArgs&, int, hipStream_t);
template int launch_w4k64p_epi<0, W4_WIDE>(GemmArgs&, int, hipStream_t);
#ifdef G4R_TOOLS_BUILD
template int launch_w4k64p_epi<2, W4_P16>(GemmArgs&, int, hipStream_t);   // the convolution over all pyramid levels (debug mode 63)
#endif

// workgroups of the persistent form = CUs of the device (one workgroup of 256 AGPRs + 128 KB LDS per CU); 256 when the query fails
int g4r_cu_count() {
  static std::atomic<int> n[64];      // per device, 0 = not asked yet
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return 256;
  int v = n[d].load(std::memory_order_relaxed);
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v <= 0) v = 256;
    n[d].store(v, std::memory_order_relaxed);
  }
  return v;
}

}  // namespace G4R_GEMM_NS
