// gemm_common.h -- what more than one GEMM kernel family uses (gemm_bf16.hip, gemm_ring.hip, gemm_pp32.hip, gemm_w4k64.hip,
// gemm_w4k64p.hip, gemv_bf16.hip): the argument block, the workgroup -> tile maps, the shared epilogues, the launchers that
// cross files and the host-side rules every launcher follows.  DESIGN.md "GEMM source map" lists file -> kernels -> tile ids.
#pragma once
#include <type_traits>

#include "g4r_common.h"

// Every file is compiled twice (bf16 and -DG4R_F16) and both objects link into one library, so whatever crosses files lives
// in a namespace that carries the dtype; hidden: nothing of it is part of the C ABI.  The kernels themselves stay in the
// anonymous namespace of their file (profile rows are matched by kernel name).
#ifdef G4R_F16
#define G4R_GEMM_NS g4r_gemm_f16
#else
#define G4R_GEMM_NS g4r_gemm_bf16
#endif
#define G4R_GEMM_NS_OPEN namespace G4R_GEMM_NS __attribute__((visibility("hidden"))) {
G4R_GEMM_NS_OPEN

struct GemmArgs {
  const h16_t* A;
  const h16_t* W;
  void* C;               // bf16 or f32 [M, ldc]
  float* ws;             // split-K partials [splits][M][N] (fp32), or null
  const float* bias;     // [N] fp32 or null
  const h16_t* residual;  // [M, ldr] bf16 or null
  const h16_t* zeros;   // >= 128 B of zeros (AMODE 1 padding source)
  long a_group_stride;   // AMODE 1: elements between groups
  int M, N, K;
  int lda, ldw, ldc, ldr;
  int act;               // 0 none, 1 relu, 2 quick_gelu (x*sigmoid(1.702x)), 3 silu,
                         // 4 swiglu: columns are interleaved (gate, up) pairs, C has N/2 columns
  int out_f32;
  int splits, tiles_per_split;  // K tiles (of 64) per z slice
  int H, Wd, Cin, groups;      // AMODE 1 geometry
  int lvl_start[5];            // AMODE 2: first row of each level's maps (lvl_start[n_lvl] = M), levels stacked [level][b][y][x]
  int lvl_h[4], lvl_w[4];      // AMODE 2: map size per level
  int n_lvl;
  int tiles_m, tiles_n;
  int n_fastest;  // tile order: 1 = consecutive workgroups walk N first (share the A / activation tile)
  int group_m;    // > 0: grouped tile order (g4r_tile_coords), row tiles per group
  int dbg;  // ablation probe (tools only): 1 = skip the loads after the first tile, 2 = skip the MFMAs
  unsigned a_bytes, w_bytes;   // extent of the A / W operands in bytes when < 2 GiB (buffer descriptors), else 0
  int defer_reduce;            // split-K: leave the fp32 partials in ws, the CALLER's next kernel combines them
  int stagger_ticks;           // one-wave-per-SIMD kernel: start offset step of the first 256 workgroups in 10 ns ticks (0 = none)
  // persistent form (gemm_bf16_w4k64p_kernel): extents in bytes of the tensors its epilogue addresses through buffer descriptors
  unsigned c_bytes, r_bytes, rq_bytes, rkv_bytes;
  int persist_any_k;           // tile_cfg 36: the persistent form whatever K (tests: one / two / three K tiles per output tile)
  // act == 5 (fused q|k|v projection of a LLaMA layer, ring ping-pong tiles only): RoPE and the KV-cache append happen in
  // the epilogue -- what g4r_rope_qkv_bf16 did in a launch of its own.  Columns [0, HD) -> rotated q rows of rope_q,
  // [HD, 2 HD) -> rotated k into the cache rows pos0 + t, [2 HD, 3 HD) -> v into the cache.  Row m = b * rope_T + t.
  h16_t* rope_q;              // [M][HD]
  h16_t* rope_k;              // cache base of this layer: + b * rope_kbatch + (pos0 + t) * rope_krow
  h16_t* rope_v;
  const float* rope_cos;       // [maxT][D/2] fp32
  const float* rope_sin;
  long rope_krow, rope_kbatch;
  int rope_T, rope_pos0, rope_HD;
};

constexpr int BK = 64;

// Workgroup -> (output tile, K slice).  The dispatcher deals consecutive linear workgroup ids (x fastest, then y) round robin
// to the 8 XCDs; each XCD has its own L2.  The map hands every XCD one CONTIGUOUS run of the virtual ids
// [slice][tile] (cdna_hip_programming.md 5.5 T1, bijective for any count): without K slices that is a run of neighbouring
// tiles; with K slices an XCD works on as few slices as possible -- many tiles of ONE K window share the A rows and the W rows
// of that window in its L2.  (Round 2 mapped tiles only and gave every XCD all the slices of a few tiles: on the LLaMA
// down_proj, 64 tiles x 4 slices, every L2 then streamed the whole A matrix, 8 x 17 MB, and the K tile ran 1.7x the qkv's.)
__device__ __forceinline__ void g4r_workgroup_tile_slice(int nwg, bool tile_major, int& tile, int& slice) {
  if (tile_major) {                        // tools only (debug mode 11): the round-2 map, for A/B runs
    const int wg = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = wg & 7, idx = wg >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    slice = blockIdx.y;
    return;
  }
  const int total = nwg * (int)gridDim.y;
  const int lin = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
  const int q = total >> 3, r = total & 7, xcd = lin & 7, idx = lin >> 3;
  const int v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  slice = v / nwg;
  tile = v - slice * nwg;
}

// Tile id -> (row tile, column tile).  group_m == 0: the plain orders (M fastest: consecutive workgroups share a W panel; N
// fastest: they share an A tile).  group_m > 0 (round 4, dense GEMMs with many row tiles): GROUPED order -- ids sweep `group_m`
// row tiles x all column tiles, M fastest inside the group -- so that the 32 workgroups an XCD runs at a time form a compact
// group_m x (32 / group_m) block of tiles instead of one column of 32 row tiles: its L2 then streams group_m A tiles + 32 /
// group_m W panels per wave instead of ALL of A (8 merged requests, 6136 x 4096 x 4096: every XCD re-read the whole 50 MB
// activation matrix for each of its waves, 1.65 GB of HBM-side reads per launch against 134 MB algorithmic,
// profiles/r04_pmc_report.txt).
__device__ __forceinline__ void g4r_tile_coords(int wg, int tiles_m, int tiles_n, int n_fastest, int group_m, int& tile_m, int& tile_n) {
  if (group_m < 0) {
    // groups of -group_m COLUMN tiles x all row tiles, N fastest inside the group (conv: few column tiles, a big W panel each)
    const int gn = -group_m;
    const int per_group = gn * tiles_m;
    const int gid = wg / per_group;
    const int first_n = gid * gn;
    const int gsz = (tiles_n - first_n) < gn ? (tiles_n - first_n) : gn;
    const int in_group = wg - gid * per_group;
    tile_n = first_n + in_group % gsz;
    tile_m = in_group / gsz;
    return;
  }
  if (group_m > 0) {
    const int per_group = group_m * tiles_n;
    const int gid = wg / per_group;
    const int first_m = gid * group_m;
    const int gsz = (tiles_m - first_m) < group_m ? (tiles_m - first_m) : group_m;
    const int in_group = wg - gid * per_group;
    tile_m = first_m + in_group % gsz;
    tile_n = in_group / gsz;
    return;
  }
  tile_m = n_fastest ? wg / tiles_n : wg % tiles_m;
  tile_n = n_fastest ? wg % tiles_n : wg / tiles_m;
}

// waves per SIMD the kernel is allowed to assume = workgroups that fit the 160 KB LDS (<= 3)
constexpr int gemm_waves_per_eu(int bm, int bn, int nw, int stages, int bk) {
  int blocks = (160 * 1024) / (stages * (bm + bn) * bk * 2);
  if (blocks > 3) blocks = 3;
  if (blocks < 1) blocks = 1;
  int w = blocks * nw / 4;
  return w > 4 ? 4 : (w < 1 ? 1 : w);
}

__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == 1) return v > 0.f ? v : 0.f;
  if (act == 2) return v / (1.f + __expf(-1.702f * v));
  if (act == 3) return v / (1.f + __expf(-v));
  return v;
}

// Shared epilogue.  acc[i][j] is the 32x32 accumulator of rows mw + 32*i.. and columns nw + 32*j..,
// in the swapped-operand layout D[n][m]: this lane holds m = mw + 32*i and, per register quad q,
// the 4 consecutive columns nw + 32*j + 8*q .. +3 (mw / nw already include the lane offsets).
// J0 / JN: the accumulator columns this call handles (a 4 x 4 wave tile is emitted as two calls of 4 x 2: the fully
// unrolled 16-accumulator nest exceeds the compiler's unroll budget, and a rolled nest would index `acc` dynamically,
// i.e. put the accumulators in scratch).
template <int TM, int TN, int J0 = 0, int JN = TN>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& p, float16v (&acc)[TM][TN], int mw, int nw,
                                              int split) {
  const bool vec_ok = (p.N & 3) == 0;  // then every in-range quad is a full, aligned quad
  if (p.splits > 1) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = J0; j < J0 + JN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = mw + i * 32, n = nw + j * 32 + q * 8;
          if (m < p.M && n < p.N) {
            float* dst = p.ws + ((size_t)split * p.M + m) * p.N + n;
            if (vec_ok) {
              *reinterpret_cast<float4v*>(dst) = float4v{acc[i][j][q * 4], acc[i][j][q * 4 + 1],
                                                         acc[i][j][q * 4 + 2], acc[i][j][q * 4 + 3]};
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (n + r < p.N) dst[r] = acc[i][j][q * 4 + r];
            }
          }
        }
    return;
  }
  // One 32x32 accumulator at a time (keeps the live range of epilogue temporaries short):
  // bias (16-B loads) -> activation (wave-uniform branch) -> residual add -> packed store.
  const bool res_vec = vec_ok && (p.ldr & 3) == 0;
  const bool out_vec = vec_ok && (p.ldc & 3) == 0;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = J0; j < J0 + JN; ++j) {
      float16v c = acc[i][j];
      const int m = mw + i * 32;
      if (p.bias) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = nw + j * 32 + q * 8;
          float4v b = {0.f, 0.f, 0.f, 0.f};
          if (n < p.N) {
            if (vec_ok) {
              b = *reinterpret_cast<const float4v*>(p.bias + n);
            } else {
              b.x = p.bias[n];
              if (n + 1 < p.N) b.y = p.bias[n + 1];
              if (n + 2 < p.N) b.z = p.bias[n + 2];
              if (n + 3 < p.N) b.w = p.bias[n + 3];
            }
          }
          c[q * 4 + 0] += b.x;
          c[q * 4 + 1] += b.y;
          c[q * 4 + 2] += b.z;
          c[q * 4 + 3] += b.w;
        }
      }
      if (p.act == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = fmaxf(c[r], 0.f);
      } else if (p.act == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = c[r] / (1.f + __expf(-1.702f * c[r]));
      } else if (p.act == 3) {
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = c[r] / (1.f + __expf(-c[r]));
      }
      if (m < p.M && p.act == 4) {
        // SwiGLU epilogue (LLaMA MLP, HF LlamaMLP: down(silu(gate(x)) * up(x))): the weight rows were
        // interleaved at prepare() so this lane's quad is (g0, u0, g1, u1); silu is rounded to bf16
        // before the product, as the un-fused reference does.
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = nw + j * 32 + q * 8;
          if (n >= p.N) continue;
          const float g0 = c[q * 4], u0 = c[q * 4 + 1], g1 = c[q * 4 + 2], u1 = c[q * 4 + 3];
          const float s0 = h16lo(pack_h16x2(g0 / (1.f + __expf(-g0)), 0.f));
          const float s1 = h16lo(pack_h16x2(g1 / (1.f + __expf(-g1)), 0.f));
          h16_t* dst = reinterpret_cast<h16_t*>(p.C) + (size_t)m * p.ldc + (n >> 1);
          *reinterpret_cast<uint32_t*>(dst) = pack_h16x2(s0 * u0, s1 * u1);
        }
      } else if (m < p.M) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = nw + j * 32 + q * 8;
          if (n >= p.N) continue;
          float v0 = c[q * 4], v1 = c[q * 4 + 1], v2 = c[q * 4 + 2], v3 = c[q * 4 + 3];
          if (p.residual) {
            const h16_t* rp = p.residual + (size_t)m * p.ldr + n;
            if (res_vec) {
              const uint2v rr = *reinterpret_cast<const uint2v*>(rp);
              v0 += h16lo(rr.x); v1 += h16hi(rr.x); v2 += h16lo(rr.y); v3 += h16hi(rr.y);
            } else {
              v0 += h16_to_f32(rp[0]);
              if (n + 1 < p.N) v1 += h16_to_f32(rp[1]);
              if (n + 2 < p.N) v2 += h16_to_f32(rp[2]);
              if (n + 3 < p.N) v3 += h16_to_f32(rp[3]);
            }
          }
          if (p.out_f32) {
            float* dst = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
            if (out_vec) {
              *reinterpret_cast<float4v*>(dst) = float4v{v0, v1, v2, v3};
            } else {
              dst[0] = v0;
              if (n + 1 < p.N) dst[1] = v1;
              if (n + 2 < p.N) dst[2] = v2;
              if (n + 3 < p.N) dst[3] = v3;
            }
          } else {
            h16_t* dst = reinterpret_cast<h16_t*>(p.C) + (size_t)m * p.ldc + n;
            if (out_vec) {
              *reinterpret_cast<uint2v*>(dst) = uint2v{pack_h16x2(v0, v1), pack_h16x2(v2, v3)};
            } else {
              dst[0] = f32_to_h16(v0);
              if (n + 1 < p.N) dst[1] = f32_to_h16(v1);
              if (n + 2 < p.N) dst[2] = f32_to_h16(v2);
              if (n + 3 < p.N) dst[3] = f32_to_h16(v3);
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Epilogue of the 256 x 256 kernels, staged through LDS (round 2).  In the swapped-operand accumulator layout a lane
// owns ONE output row m and scattered column quads, so the direct epilogue above issues stores of 64 x 8 bytes on 32
// different rows: every store instruction touches 32-64 cache lines with 8 bytes each.  Measured: ~20 us of a ~105 us
// K = 4096 launch outside the K loop (profiles/r02_gemm_tiles.md).  Here each wave parks its accumulators (fp32, 64 rows at
// a time) in its own slice of the -- now idle -- operand ring and reads them back ROW-major: 8 consecutive columns per
// lane, WTN/8 lanes per row, so every store / bias / residual access is a whole 16-byte (bf16) or 32-byte (fp32) run of
// one row and a wave instruction covers complete 128-byte lines.  The arithmetic and its order are those of
// gemm_epilogue (bias -> activation -> residual -> one rounding), so results are bit-identical to the direct path.
// ---------------------------------------------------------------------------------------------
template <int TN, int PR = 64>
struct EpiLds {
  static constexpr int WTN = 32 * TN;            // wave-tile columns
  static constexpr int RS = WTN * 4 + 16;        // row stride in bytes (fp32 row + 16 B: conflict-free b128 writes)
  static constexpr int WAVE_BYTES = PR * RS;     // PR (32 or 64) rows per pass
};

template <int TM, int TN, int PR = 64>
__device__ __forceinline__ void gemm_epilogue_lds(const GemmArgs& p, float16v (&acc)[TM][TN], char* wave_lds, int m_wave0,
                                                  int n_wave0, int lane, int split) {
  using E = EpiLds<TN, PR>;
  constexpr int LPR = E::WTN / 8;                // lanes per row (8 columns each)
  constexpr int RPI = 64 / LPR;                  // rows per wave instruction (WTN = 96: 5 rows, 4 lanes idle)
  constexpr int BPP = PR / 32;                   // 32-row accumulator blocks per pass
  constexpr int NIT = (PR + RPI - 1) / RPI;      // read-back iterations per pass
  static_assert((TM * 32) % PR == 0, "pass geometry");
  const int wr = lane & 31, wh = lane >> 5;
  const int rrow = lane / LPR, rcol = (lane % LPR) * 8;
  const bool vec_n = (p.N & 7) == 0;
  const bool swiglu = p.act == 4;
#pragma unroll
  for (int half = 0; half < TM / BPP; ++half) {
    // ---- park PR rows: lane writes its 4-column quads (16-byte LDS stores, rows = lanes) ----
#pragma unroll
    for (int i2 = 0; i2 < BPP; ++i2)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float16v& c = acc[half * BPP + i2][j];
          *reinterpret_cast<float4v*>(wave_lds + (i2 * 32 + wr) * E::RS + (j * 32 + q * 8 + wh * 4) * 4) =
              float4v{c[q * 4], c[q * 4 + 1], c[q * 4 + 2], c[q * 4 + 3]};
        }
    if (p.act == 5) {
      // ---- fused RoPE + KV-cache append (head_dim 128: this wave's 64 columns are HALF a head, the other half sits in
      //      the LDS slice of the neighbouring wave, same rows, same lane -> column map) ----
      if constexpr (E::WTN == 64) {
        __syncthreads();                                     // every wave has parked this pass
        const int wave_id = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const char* mate_lds = wave_lds + ((wave_id & 1) ? -E::WAVE_BYTES : E::WAVE_BYTES);
        const int part = n_wave0 / p.rope_HD;                // 0 q, 1 k, 2 v (a 256-column tile never straddles: HD % 256 == 0)
        const bool second = (wave_id & 1) != 0;              // this wave holds d in [64, 128) of its head
#pragma unroll 2
        for (int it = 0; it < NIT; ++it) {
          const int r = it * RPI + rrow;
          if (rrow >= RPI || r >= PR) continue;
          const int m = m_wave0 + half * PR + r;
          if (m >= p.M) continue;
          const float4v a0 = *reinterpret_cast<const float4v*>(wave_lds + r * E::RS + rcol * 4);
          const float4v a1 = *reinterpret_cast<const float4v*>(wave_lds + r * E::RS + rcol * 4 + 16);
          float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
          const int b = m / p.rope_T, t = m - b * p.rope_T;
          const int pos = p.rope_pos0 + t;
          const int col = n_wave0 + rcol - part * p.rope_HD;   // column inside q / k / v
          // the unfused path stored the projection as bf16 before rotating it: keep that rounding point
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = h16_to_f32(f32_to_h16(v[k]));
          if (part < 2) {
            const float4v m0 = *reinterpret_cast<const float4v*>(mate_lds + r * E::RS + rcol * 4);
            const float4v m1 = *reinterpret_cast<const float4v*>(mate_lds + r * E::RS + rcol * 4 + 16);
            float u[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
            const float* cp = p.rope_cos + (size_t)pos * 64 + rcol;
            const float* sp = p.rope_sin + (size_t)pos * 64 + rcol;
            const float4v c0 = *reinterpret_cast<const float4v*>(cp), c1 = *reinterpret_cast<const float4v*>(cp + 4);
            const float4v s0 = *reinterpret_cast<const float4v*>(sp), s1 = *reinterpret_cast<const float4v*>(sp + 4);
            const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
            const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const float mate = h16_to_f32(f32_to_h16(u[k]));
              // rotate_half: first half  a' = a cos - b sin ; second half  b' = b cos + a sin   (a = x[d], b = x[d + 64])
              v[k] = second ? __builtin_fmaf(v[k], cs[k], mate * sn[k]) : __builtin_fmaf(v[k], cs[k], -(mate * sn[k]));
            }
          }
          h16_t* dst = part == 0 ? p.rope_q + (size_t)m * p.rope_HD + col
                                  : (part == 1 ? p.rope_k : p.rope_v) + (size_t)b * p.rope_kbatch + (size_t)pos * p.rope_krow + col;
          *reinterpret_cast<uint4v*>(dst) = uint4v{pack_h16x2(v[0], v[1]), pack_h16x2(v[2], v[3]), pack_h16x2(v[4], v[5]),
                                                   pack_h16x2(v[6], v[7])};
        }
        __syncthreads();                                     // the neighbour is done with this wave's slice
      }
      continue;
    }
    // ---- read back row-major and finish ----
#pragma unroll 2
    for (int it = 0; it < NIT; ++it) {
      const int r = it * RPI + rrow;
      if (rrow >= RPI || r >= PR) continue;      // idle lanes / the last, partial iteration (no barrier inside the loop)
      const int m = m_wave0 + half * PR + r, n = n_wave0 + rcol;
      const float4v a0 = *reinterpret_cast<const float4v*>(wave_lds + r * E::RS + rcol * 4);
      const float4v a1 = *reinterpret_cast<const float4v*>(wave_lds + r * E::RS + rcol * 4 + 16);
      if (m >= p.M || n >= p.N) continue;
      float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const int nv = p.N - n < 8 ? p.N - n : 8;           // valid columns of this run
      if (p.splits > 1) {
        float* dst = p.ws + ((size_t)split * p.M + m) * p.N + n;
        if (nv == 8 && vec_n) {
          *reinterpret_cast<float4v*>(dst) = a0;
          *reinterpret_cast<float4v*>(dst + 4) = a1;
        } else {
          for (int k = 0; k < nv; ++k) dst[k] = v[k];
        }
        continue;
      }
      if (p.bias) {
        if (nv == 8 && vec_n) {
          const float4v b0 = *reinterpret_cast<const float4v*>(p.bias + n), b1 = *reinterpret_cast<const float4v*>(p.bias + n + 4);
          v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
        } else {
          for (int k = 0; k < nv; ++k) v[k] += p.bias[n + k];
        }
      }
      if (p.act == 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
      } else if (p.act == 2) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = v[k] / (1.f + __expf(-1.702f * v[k]));
      } else if (p.act == 3) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = v[k] / (1.f + __expf(-v[k]));
      }
      if (swiglu) {
        // (gate, up) column pairs -> N/2 output columns (the launcher guarantees N % 4 == 0, bf16 out, no bias/residual)
        h16_t* dst = reinterpret_cast<h16_t*>(p.C) + (size_t)m * p.ldc + (n >> 1);
        uint32_t w2[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float g0 = v[4 * k], u0 = v[4 * k + 1], g1 = v[4 * k + 2], u1 = v[4 * k + 3];
          const float s0 = h16lo(pack_h16x2(g0 / (1.f + __expf(-g0)), 0.f));
          const float s1 = h16lo(pack_h16x2(g1 / (1.f + __expf(-g1)), 0.f));
          w2[k] = pack_h16x2(s0 * u0, s1 * u1);
        }
        if (nv == 8 && (p.ldc & 3) == 0) {
          *reinterpret_cast<uint2v*>(dst) = uint2v{w2[0], w2[1]};
        } else {
          *reinterpret_cast<uint32_t*>(dst) = w2[0];
          if (nv > 4) *reinterpret_cast<uint32_t*>(dst + 2) = w2[1];
        }
        continue;
      }
      if (p.residual) {
        const h16_t* rp = p.residual + (size_t)m * p.ldr + n;
        if (nv == 8 && vec_n && (p.ldr & 7) == 0) {
          const uint4v rr = *reinterpret_cast<const uint4v*>(rp);
          v[0] += h16lo(rr.x); v[1] += h16hi(rr.x); v[2] += h16lo(rr.y); v[3] += h16hi(rr.y);
          v[4] += h16lo(rr.z); v[5] += h16hi(rr.z); v[6] += h16lo(rr.w); v[7] += h16hi(rr.w);
        } else {
          for (int k = 0; k < nv; ++k) v[k] += h16_to_f32(rp[k]);
        }
      }
      if (p.out_f32) {
        float* dst = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
        if (nv == 8 && vec_n && (p.ldc & 3) == 0) {
          *reinterpret_cast<float4v*>(dst) = float4v{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<float4v*>(dst + 4) = float4v{v[4], v[5], v[6], v[7]};
        } else {
          for (int k = 0; k < nv; ++k) dst[k] = v[k];
        }
      } else {
        h16_t* dst = reinterpret_cast<h16_t*>(p.C) + (size_t)m * p.ldc + n;
        if (nv == 8 && vec_n && (p.ldc & 7) == 0) {
          *reinterpret_cast<uint4v*>(dst) = uint4v{pack_h16x2(v[0], v[1]), pack_h16x2(v[2], v[3]), pack_h16x2(v[4], v[5]),
                                                   pack_h16x2(v[6], v[7])};
        } else {
          for (int k = 0; k < nv; ++k) dst[k] = f32_to_h16(v[k]);
        }
      }
    }
  }
}

// Workgroup barrier of the kernels whose two wave groups run out of phase (ring ping-pong): LDS reads drained first, and the
// compiler may move nothing across it.
#define G4R_PP_BARRIER()                                   \
  do {                                                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     \
    __builtin_amdgcn_sched_barrier(0);                     \
    __builtin_amdgcn_s_barrier();                          \
    __builtin_amdgcn_sched_barrier(0);                     \
  } while (0)

// one 1 KiB LDS-DMA piece as buffer_load_dwordx4 ... lds: descriptor over `base`, per-lane byte offset, scalar byte offset.
// (A free __device__ function: the same builtins written inside a lambda of the kernel make hipcc drop the kernel's host
// handle -- the lambda is implicitly __host__ __device__ and the builtin does not exist on the host.)
__device__ __forceinline__ void g4r_buffer_piece(const void* base, unsigned bytes, void* lds, int voff, int soff) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
}

// epilogue modes of the one-wave-per-SIMD kernels (gemm_w4k64.hip states them; the launcher picks one)
enum { W4_GENERIC = 0, W4_P16 = 1, W4_SWIGLU = 2, W4_ROPE = 3, W4_WIDE = 4 };

// One accumulator register -> VGPR, in program order.  Without it the compiler copies all 256 AGPRs to VGPRs at the head of
// the epilogue (v_accvgpr_read x 256 -> 548 bytes of scratch per lane); the volatile asm keeps every value in its AGPR until
// the park loop reaches it.
__device__ __forceinline__ float w4_acc(const float16v& c, int r) {
  float v;
  asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(c[r]));
  return v;
}

// ---- host side ---------------------------------------------------------------------------------------------------
extern int g_gemm_dbg;   // tools only: ablation / A-B probe modes (g4r_gemm_debug_mode; the fp16 copy is never set)

// split-K geometry in units of the launching kernel's K tile: K tiles per slice, and the slices that leaves
inline void gemm_split_geometry(GemmArgs& p, int bkt) {
  const int nt = p.K / bkt;
  int splits = p.splits < 1 ? 1 : p.splits;
  if (splits > nt) splits = nt;
  p.tiles_per_split = g4r_ceil_div(nt, splits);
  p.splits = g4r_ceil_div(nt, p.tiles_per_split);
}

// every split-K launcher ends with this: the combine launch (splitk_reduce_kernel, gemm_bf16.hip) unless there is one slice
// or the caller's next kernel combines the partials (defer_reduce)
int gemm_reduce_tail(GemmArgs& p, hipStream_t stream);

// dynamic LDS above 64 KB: raise the kernel's limit once per device (`once`: one static per kernel instantiation); a failing
// call leaves the device un-marked so that the next launch tries again
inline int gemm_raise_lds_limit(G4rPerDeviceOnce& once, const void* kern, size_t lds, const char* where) {
  if (!once.first()) return G4R_OK;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) return G4R_OK;
  once.failed();
  return g4r_note_hip_error(e, where);
}

// The launchers gemm_bf16.hip's tile switch and entry points call; each family file instantiates the forms named there.
template <int BM, int BN, int WM, int WN, int AMODE, bool GLDS, int STAGES = 2, int BKT = 64, int STYLE = 0>
int launch_tile(GemmArgs& p, hipStream_t stream);                                   // gemm_ring.hip
template <int AMODE, bool PROBE = false, int BM = 256, int BN = 256, bool BUF = true, int SCHED = 0>
int launch_pp32(GemmArgs& p, hipStream_t stream);                                   // gemm_pp32.hip
template <int AMODE, bool PROBE = false>
int launch_w4k64(GemmArgs& p, hipStream_t stream);                                  // gemm_w4k64.hip
template <int AMODE, int EPI>
int launch_w4k64p_epi(GemmArgs& p, int grid, hipStream_t stream);                   // gemm_w4k64p.hip
int g4r_cu_count();                                                                 // gemm_w4k64p.hip

// gemv_bf16.hip: x is staged in dynamic LDS (2 K bytes) next to a 16-byte static array: both must fit the default 64 KB limit
#define G4R_GEMV_MAX_K 32736
void gemv_dispatch(int variant, int xmode, const h16_t* x, const float* gamma, float eps, int mS, int mD, const h16_t* W,
                   void* C, const float* bias, const h16_t* residual, int N, int K, int ldw, int act, int out_f32,
                   hipStream_t st);

}  // namespace G4R_GEMM_NS
using namespace G4R_GEMM_NS;
