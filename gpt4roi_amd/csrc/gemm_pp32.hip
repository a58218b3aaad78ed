// gemm_pp32.hip -- the ring ping-pong kernel (gemm_bf16_pp32_kernel): tiles 24 and 28 of launch_gemm's switch (gemm_bf16.hip),
// the fallback of tile 34 for operands of 2 GiB and more and, in the tools build, tiles 25, 27, 30, 31, 33.
#include "gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Ping-pong kernel, second form: K tiles of 32 in a RING OF FOUR (4 x 32 KB of LDS), one phase per K tile.
// A stamped run of the first form (K tiles of 64, four barriers per tile; removed) showed that the LDS-DMA address path is the co-limiter: a CU
// accepts one 1 KiB piece every ~26 cycles, i.e. 1664 cycles of issue per 64 of K against 2048 cycles of MFMA,
// and a wave that is issuing pieces cannot issue MFMAs.  So here ONLY the group that is reading fragments issues
// pieces (its 4 per K tile, for the tile three ahead: 16 pieces = ~416 cycles per phase, under the other group's
// 16 MFMAs), never the group on the matrix pipe, and every wave has five phases of slack for its pieces to land:
//        phase:     2t              2t+1            2t+2
//   waves 0-3:   read(t)+DMA(t+3)   MFMA(t)      read(t+1)+DMA(t+4)
//   waves 4-7:   MFMA(t-1)          read(t)+DMA(t+3)   MFMA(t)
// ---------------------------------------------------------------------------------------------
// BM x BN = 256 x 256 (wave tile 128 x 64) or 128 x 384 (wave tile 64 x 96: 6 x 32 = 192 workgroups for the LLaMA fused-qkv
// shape 767 x 12288, where 256 x 256 tiles give only 144 of the 256 CUs a tile); both stage 32 KB per K tile = 4 LDS-DMA
// pieces per wave, so the ring, the waits and the phase structure are identical.
// (Round-3 probes, since removed: issuing a wave's W pieces -- or all four -- at the HEAD of its MFMA phase instead of the end
// of its read phase changes nothing with global_load_lds pieces (4096^3 1174 / 1141 / 1153 TF/s back to back, conv 192^2
// 860 / 859 / 739; profiles/r03_gemm_bench_a.jsonl) and loses 5 % with the buffer form below (1153 -> 1098; conv 1013 ->
// 895); a piece after every fourth MFMA is 14x slower.  In-kernel stamps with the buffer form: fragment reads 220-300
// cycles + 4 pieces 260-270 (the 16 pieces of a group now go out at the vector-memory path's 16 cycles each) + 92 + 85 of
// wait / barrier = ~670 against 512 + ~60 for the MFMA phase: 1410 cycles per K = 32 tile, was 1481.)
// BUF (round 3, the default): the pieces are buffer_load_dwordx4 ... lds through a buffer descriptor -- a 32-bit per-lane
// byte offset computed once + a scalar K / tap offset per tile -- instead of global_load_lds with 64-bit per-lane
// addresses: one SALU add (M0) and one VMEM instruction per piece, no VALU in the read phase for the dense case.  An
// out-of-image conv tap is an offset beyond the descriptor's num_records, which the hardware returns as zeros (no zero
// line, no 64-bit select).  Measured (tools/gemm_bench.cpp, burst arm): 4096^3 1101 -> 1157 TF/s, 8192^2 x 4096
// 1099 -> 1186, the 144-workgroup qkv launch 767 x 12288 x 4096 106.5 -> 88.1 us.  BUF = false (global_load_lds) remains
// for operands of 2 GiB and more, which a 32-bit offset cannot span.
// SCHED 1 (round 3): ONE barrier per K tile and the two groups' loop bodies rotated against each other,
//        interval k:   group 0:  read(k)  pieces(k+3)  MFMA(k)            | vmcnt, barrier
//                      group 1:  MFMA(k-1)  read(k)  pieces(k+3)          | vmcnt, barrier
// instead of the two barriers per tile of SCHED 0, which lock the groups into "one reads while the other multiplies"
// slots of max(read phase, MFMA phase) = ~705 cycles each (1410 per tile; the read phase, ~670, is the longer one).
// Here a wave's tile costs read + MFMA = ~1180 of its own time and the other wave of its SIMD has its MFMAs exactly
// where this one reads (group 1 multiplies tile k-1 during group 0's read of tile k, group 0 multiplies tile k during
// group 1's read of it).  Prefetch distance 2 in the ring of 4: the pieces of tile k+2 overwrite the buffer of tile k-2,
// whose last reads were two barriers ago for BOTH groups; tile k's pieces were waited for (counted vmcnt, leaving only
// tile k+1's in flight) before barrier k by every wave.
// Round 4: eight further schedules and structures of this K loop, and the ablations of the shipped one (debug modes 21-26), were
// measured and removed again; DESIGN.md section 3 "Round 4" has the table, and why round 5 read it differently (gemm_w4k64.hip).
template <int AMODE, bool PROBE = false, int BM = 256, int BN = 256, bool BUF = true, int SCHED = 0>
__global__ __launch_bounds__(512, 2) void gemm_bf16_pp32_kernel(GemmArgs p) {
  constexpr int NW = 8, NT = 512, BKT = 32, RING = 4;
  constexpr int ROWB = 64, SPR = 4;
  constexpr int WTM = BM / 2, WTN = BN / 4;      // wave tile: 2 row groups (the two ping-pong groups) x 4 column slices
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert((BM + BN == 512 || (BM == 192 && BN == 256)) && WTM % 32 == 0 && WTN % 32 == 0,
                "32 KB (28 KB for 192 x 256) per K tile, 32x32 accumulator blocks");
  // pieces per wave per K tile: 2 + 2; for BM = 192 the A tile has 12 pieces -> waves 0-3 carry two, waves 4-7 one
  constexpr int NA = (BM * SPR + NT - 1) / NT, NB = BN * SPR / NT;
  constexpr bool UNEVEN = (BM * SPR) % NT != 0;
  constexpr int A_BYTES = BM * BKT * 2, STAGE_BYTES = (BM + BN) * BKT * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // RING * STAGE_BYTES = 128 KB
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int grp = wm;
  const int nwg = p.tiles_m * p.tiles_n;
  int wg, split;
  g4r_workgroup_tile_slice(nwg, p.dbg == 11, wg, split);
  int tile_m, tile_n;
  g4r_tile_coords(wg, p.tiles_m, p.tiles_n, p.n_fastest, p.group_m, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  // tools only (ablations of the K loop; results are wrong by construction): dbg 21 = every workgroup streams the operands
  // of tile (0, 0) -- an L2-resident 4 MB working set, so what remains is the CU's own load path; 22 = no pieces after the
  // ring fill (MFMA + fragment reads only); 23 = no MFMAs (loads + fragment reads only); 24 = no fragment reads either
  const int lm0 = p.dbg == 21 ? 0 : m0, ln0 = p.dbg == 21 ? 0 : n0;
  const int t_begin = split * p.tiles_per_split;
  int t_end = t_begin + p.tiles_per_split;
  const int nt_total = p.K / BKT;
  if (t_end > nt_total) t_end = nt_total;
  // PROBE (tools/pp32_probe3.py): every workgroup's wave 0 records entry / loop begin / loop end / exit (s_memtime) and
  // its XCC id at ws + 16 + 8 * blockIdx.x  (int64)
  long long* wg_stamps = reinterpret_cast<long long*>(p.ws) + 16 + 8 * (long)blockIdx.x;
  const bool wg_probe = PROBE && blockIdx.y == 0 && wave == 0 && lane == 0;
  if (PROBE) { if (wg_probe) { wg_stamps[0] = __builtin_amdgcn_s_memtime(); wg_stamps[4] = __builtin_amdgcn_s_getreg(6164); wg_stamps[5] = wall_clock64(); } }

  const h16_t* a_src[NA];
  int a_y[NA], a_x[NA];
  int a_h[NA], a_w[NA];                    // AMODE 2: the row's own map size (rows of several pyramid levels in one GEMM)
  unsigned a_ok[NA];
  int a_pitch[NA];
  const h16_t* b_src[NB];
  int a_voff[NA], b_voff[NB];              // BUF: byte offsets of this lane's 16 bytes from the matrix base (k = 0)
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int pslot = (j * NW + wave) * 64 + lane;
    // tools only, dbg 25 / 26: every piece reads 8 rows x 128 B (whole cache lines) instead of 16 rows x 64 B (half lines)
    const bool full_lines = p.dbg == 25 || p.dbg == 26;
    const int row = full_lines ? pslot / 8 : pslot / SPR, ps = full_lines ? pslot % 8 : pslot % SPR;
    const int kslot = full_lines ? ps : ps ^ ((row >> 2) & 3);
    int gm = lm0 + row;
    if (gm > p.M - 1) gm = p.M - 1;
    a_src[j] = p.A + (size_t)gm * p.lda + kslot * 8;
    a_voff[j] = (gm * p.lda + kslot * 8) * 2;
    a_y[j] = a_x[j] = 0;
    a_h[j] = p.H; a_w[j] = p.Wd;
    if (AMODE == 2) {
      int lv = 0;
#pragma unroll
      for (int q = 1; q < 4; ++q)
        if (q < p.n_lvl && gm >= p.lvl_start[q]) lv = q;
      a_h[j] = p.lvl_h[lv]; a_w[j] = p.lvl_w[lv];
      const int local = gm - p.lvl_start[lv];
      const int hw = a_h[j] * a_w[j];
      const int rem = local - (local / hw) * hw;
      a_y[j] = rem / a_w[j];
      a_x[j] = rem - a_y[j] * a_w[j];
    }
    if (AMODE == 1) {
      const int hw = p.H * p.Wd;
      const int b = gm / hw, rem = gm - b * hw;
      a_y[j] = rem / p.Wd;
      a_x[j] = rem - a_y[j] * p.Wd;
    }
    // the nine taps' in-image bits of this lane's pixel and its row pitch in elements: the per-K-tile work of a piece is
    // then one bit test, one multiply-add and a select (the four compares and the 64-bit multiply per piece per K tile of
    // round 2 sat in the READ phase, the longer one of the ping-pong: the conv's K tile ran 1.3x the dense GEMM's)
    a_ok[j] = 0;
    a_pitch[j] = a_w[j] * p.lda;
    if (AMODE >= 1) {
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int yy = a_y[j] + tp / 3 - 1, xx = a_x[j] + tp % 3 - 1;
        if (yy >= 0 && yy < a_h[j] && xx >= 0 && xx < a_w[j]) a_ok[j] |= 1u << tp;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int pslot = (j * NW + wave) * 64 + lane;
    const bool full_lines = p.dbg == 25 || p.dbg == 26;
    const int row = full_lines ? pslot / 8 : pslot / SPR, ps = full_lines ? pslot % 8 : pslot % SPR;
    const int kslot = full_lines ? ps : ps ^ ((row >> 2) & 3);
    int gn = ln0 + row;
    if (gn > p.N - 1) gn = p.N - 1;
    b_src[j] = p.W + (size_t)gn * p.ldw + kslot * 8;
    b_voff[j] = (gn * p.ldw + kslot * 8) * 2;
  }
  struct TileSrc { long a_off; int k0, dy, dx, tap, shift, soff; };   // shift / soff: the BUF form of a_off (elements / bytes)
  // (channel slice, group, tap) of the NEXT tile to stage: tiles are staged strictly in order, so the walk is a counter
  // (taps fastest, then groups, then 32-channel slices) instead of two runtime divisions per K tile per wave
  int st_ct = 0, st_g = 0, st_tap = 0;
  if (AMODE >= 1) {
    const int n_taps = 9 * p.groups;
    st_ct = t_begin / n_taps;
    const int rem = t_begin - st_ct * n_taps;
    st_g = rem / 9;
    st_tap = rem - st_g * 9;
  }
  auto tile_src = [&](int t) {
    TileSrc ts;
    ts.k0 = t * BKT;
    if (p.dbg == 25 || p.dbg == 26) ts.k0 = ((t * 64) % (p.K - 63)) & ~63;
    ts.a_off = ts.k0;
    ts.dy = ts.dx = ts.tap = ts.shift = 0;
    ts.soff = ts.k0 * 2;
    if (AMODE >= 1) {
      const int c0 = st_ct * BKT;
      ts.tap = st_tap;
      ts.dy = st_tap / 3 - 1;
      ts.dx = st_tap - (st_tap / 3) * 3 - 1;
      ts.a_off = (long)st_g * p.a_group_stride + (long)((ts.dy * p.Wd + ts.dx) * p.lda) + c0;
      if (AMODE == 2) ts.a_off = c0;            // the pixel shift depends on the row's own map width: added per piece
      // buffer form: the (possibly negative) pixel shift goes into the per-lane offset, the scalar offset stays >= 0
      ts.shift = AMODE == 2 ? 0 : (ts.dy * p.Wd + ts.dx) * p.lda;
      ts.soff = (int)(((long)st_g * p.a_group_stride + c0) * 2);
      ts.k0 = (st_g * 9 + st_tap) * p.Cin + c0;
      if (++st_tap == 9) {
        st_tap = 0;
        if (++st_g == p.groups) { st_g = 0; ++st_ct; }
      }
    }
    return ts;
  };
  // piece j of a K tile for this wave: j < NA -> rows of A, else rows of W (1 KiB each)
  auto piece = [&](int j, const TileSrc& ts, int buf) {
    char* sa = smem + buf * STAGE_BYTES;
    if (j < NA) {
      if (UNEVEN && (j * NW + wave) * 16 >= BM) return;        // this wave has no j-th A piece (wave-uniform)
      if (BUF) {
        int voff = a_voff[j];
        if (AMODE == 1) voff += ts.shift * 2;
        if (AMODE == 2) voff += (ts.dy * a_pitch[j] + ts.dx * p.lda) * 2;
        if (AMODE >= 1 && !((a_ok[j] >> ts.tap) & 1u)) voff = (int)0x80000000;      // beyond num_records: reads as zeros
        g4r_buffer_piece(p.A, p.a_bytes, sa + (j * NW + wave) * 1024, voff, ts.soff);
        return;
      }
      const h16_t* src = a_src[j] + ts.a_off;
      if (AMODE == 2) src += ts.dy * a_pitch[j] + ts.dx * p.lda;
      if (AMODE >= 1) {
        if (!((a_ok[j] >> ts.tap) & 1u)) src = p.zeros + (lane & 3) * 8;
      }
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(sa + (j * NW + wave) * 1024), 16, 0, 0);
    } else {
      if (BUF) {
        g4r_buffer_piece(p.W, p.w_bytes, sa + A_BYTES + ((j - NA) * NW + wave) * 1024, b_voff[j - NA], ts.k0 * 2);
        return;
      }
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[j - NA] + ts.k0),
                                       (__attribute__((address_space(3))) void*)(sa + A_BYTES + ((j - NA) * NW + wave) * 1024), 16, 0, 0);
    }
  };
  auto stage = [&](int t, int buf) {
    const TileSrc ts = tile_src(t);
#pragma unroll
    for (int j = 0; j < NA + NB; ++j) piece(j, ts, buf);
  };
  float16v acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int frow = lane & 31, fsw = (frow >> 2) & 3, fhi = lane >> 5;
  const int a_row_off = (wm * WTM + frow) * ROWB;
  const int b_row_off = (wn * WTN + frow) * ROWB;
  h16x8 af[2][TM], wf[2][TN];
  // the 2 x (TM + TN) fragment reads of a K tile in three chunks
  auto ldchunk = [&](int buf, int c) {
    const char* sa = smem + buf * STAGE_BYTES;
    const char* sb = sa + A_BYTES;
    const int s0 = ((0 * 2 + fhi) ^ fsw) << 4, s1 = ((1 * 2 + fhi) ^ fsw) << 4;
    if (c == 0) {
#pragma unroll
      for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const h16x8*>(sa + a_row_off + i * 32 * ROWB + s0);
    } else if (c == 1) {
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[0][j] = *reinterpret_cast<const h16x8*>(sb + b_row_off + j * 32 * ROWB + s0);
#pragma unroll
      for (int i = 0; i < TM / 2; ++i) af[1][i] = *reinterpret_cast<const h16x8*>(sa + a_row_off + i * 32 * ROWB + s1);
    } else {
#pragma unroll
      for (int i = TM / 2; i < TM; ++i) af[1][i] = *reinterpret_cast<const h16x8*>(sa + a_row_off + i * 32 * ROWB + s1);
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[1][j] = *reinterpret_cast<const h16x8*>(sb + b_row_off + j * 32 * ROWB + s1);
    }
  };
  auto mma = [&]() {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = G4R_MFMA_32X32X16(wf[k2][j], af[k2][i], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  const int nt = t_end - t_begin;
  if (SCHED == 1 && nt > 0) {
#pragma unroll
    for (int t = 0; t < RING - 1; ++t)
      if (t < nt) stage(t_begin + t, t);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    auto tail_wait = [&](int i) {          // end of interval i: tile i+1 has landed (tiles i+2, i+3 may still be in flight)
      if (i + RING - 1 < nt) {
        if (UNEVEN && wave >= 4) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    };
    if (grp == 0) {
      for (int i = 0; i < nt; ++i) {
        const int buf = i & (RING - 1);
        ldchunk(buf, 0);
        ldchunk(buf, 1);
        ldchunk(buf, 2);
        if (i + RING - 1 < nt) stage(t_begin + i + RING - 1, (i + RING - 1) & (RING - 1));
        mma();
        tail_wait(i);
        G4R_PP_BARRIER();
      }
      G4R_PP_BARRIER();                    // group 1's last interval (its MFMAs of the last tile)
    } else {
      for (int i = 0; i <= nt; ++i) {
        if (i > 0) mma();                  // tile i-1: fragments read in the previous interval
        if (i < nt) {
          const int buf = i & (RING - 1);
          ldchunk(buf, 0);
          ldchunk(buf, 1);
          ldchunk(buf, 2);
          if (i + RING - 1 < nt) stage(t_begin + i + RING - 1, (i + RING - 1) & (RING - 1));
        }
        tail_wait(i);
        G4R_PP_BARRIER();
      }
    }
  }
  if (SCHED == 0 && nt > 0) {
#pragma unroll
    for (int t = 0; t < RING - 1; ++t)
      if (t < nt) stage(t_begin + t, t);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (grp == 1) G4R_PP_BARRIER();
    long long* stamps = reinterpret_cast<long long*>(p.ws) + grp * 8;
    const bool probing = PROBE && blockIdx.x == 0 && blockIdx.y == 0 && (wave & 3) == 0 && lane == 0;
#define G4R_PP32_STAMP(slot) \
  if (PROBE) { if (probing && (i == 16 || (slot) >= 6)) stamps[slot] = __builtin_amdgcn_s_memtime(); }
    {
      const int i = 0;
      G4R_PP32_STAMP(6);
    }
    if (PROBE) { if (wg_probe) wg_stamps[1] = __builtin_amdgcn_s_memtime(); }
    for (int i = 0; i < nt; ++i) {
      const int buf = i & (RING - 1);
      G4R_PP32_STAMP(0);
      // read phase of K tile i: fragments, then this wave's 4 pieces of tile i+3 into the buffer that tile i-1
      // left (both groups finished reading it: group 1 one phase ago, group 0 two)
      // fragments first, pieces after.  Alternating them inside the wave is much slower (2150-2220 vs 1490 cycles
      // per K tile, with the builtin AND with raw-ISA pieces the compiler cannot see): a ds_read behind an LDS-DMA
      // piece of the same wave waits for it in hardware.
      if (p.dbg != 24 && p.dbg != 25) {
        ldchunk(buf, 0);
        ldchunk(buf, 1);
        ldchunk(buf, 2);
      }
      G4R_PP32_STAMP(1);
      if (i + RING - 1 < nt && p.dbg != 22) {
        stage(t_begin + i + RING - 1, (i + RING - 1) & (RING - 1));
        G4R_PP32_STAMP(2);
        // tile i+1's pieces (issued two read phases ago) have landed: all but the two youngest tiles' pieces are waited for
        if (UNEVEN && wave >= 4) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      G4R_PP32_STAMP(3);
      G4R_PP_BARRIER();
      G4R_PP32_STAMP(4);
      if (p.dbg != 23 && p.dbg != 24 && p.dbg != 25) mma();
      G4R_PP_BARRIER();
      G4R_PP32_STAMP(5);
    }
    {
      const int i = 0;
      G4R_PP32_STAMP(7);
    }
    if (PROBE) { if (wg_probe) wg_stamps[2] = __builtin_amdgcn_s_memtime(); }
    if (grp == 0) G4R_PP_BARRIER();
  }
  __syncthreads();   // every wave is done with the operand ring: its space now stages the epilogue
  constexpr int EPR = (TN == 2 && TM % 2 == 0) ? 64 : 32;   // rows per epilogue pass: 8 waves x pass must fit the 160 KB of LDS
  gemm_epilogue_lds<TM, TN, EPR>(p, acc, smem + wave * EpiLds<TN, EPR>::WAVE_BYTES, m0 + wm * WTM, n0 + wn * WTN, lane, split);
  if (PROBE) { if (wg_probe) { wg_stamps[3] = __builtin_amdgcn_s_memtime(); wg_stamps[6] = wall_clock64(); } }
}

}  // namespace

G4R_GEMM_NS_OPEN

template <int AMODE, bool PROBE, int BM, int BN, bool BUF, int SCHED>
int launch_pp32(GemmArgs& p, hipStream_t stream) {
  if (BUF) {
    // extents for the buffer descriptors: the last byte a clamped row / in-image tap can touch
    size_t ab = (size_t)p.M * p.lda * 2, wb = (size_t)p.N * p.ldw * 2;
    if (AMODE == 1) ab = ((size_t)(p.groups - 1) * p.a_group_stride + (size_t)p.M * p.lda) * 2;
    if (ab >= 0x7fffffffu || wb >= 0x7fffffffu || g_gemm_dbg == 8) return launch_pp32<AMODE, PROBE, BM, BN, false, SCHED>(p, stream);
    p.a_bytes = (unsigned)ab;
    p.w_bytes = (unsigned)wb;
  }
  gemm_split_geometry(p, 32);
  p.tiles_m = g4r_ceil_div(p.M, BM);
  p.tiles_n = g4r_ceil_div(p.N, BN);
  constexpr int TN = BN / 4 / 32, TM = BM / 2 / 32;
  const size_t ring = 4 * (BM + BN) * 32 * 2, epi = 8 * (size_t)EpiLds<TN, ((TN == 2 && TM % 2 == 0) ? 64 : 32)>::WAVE_BYTES;
  const size_t lds = ring > epi ? ring : epi;
  auto kern = gemm_bf16_pp32_kernel<AMODE, PROBE, BM, BN, BUF, SCHED>;
  static G4rPerDeviceOnce attr_set;
  if (int rc = gemm_raise_lds_limit(attr_set, reinterpret_cast<const void*>(kern), lds, "gemm_pp32: hipFuncSetAttribute")) return rc;
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n, p.splits), dim3(512), lds, stream, p);
  G4R_CHECK_LAUNCH("gemm_bf16_pp32");
  return gemm_reduce_tail(p, stream);
}

// the forms the tile switch, g4r_conv3x3_mlvl_nhwc_bf16 and launch_w4k64's fallback name (each BUF form brings its own
// global_load_lds form along)
#define G4R_PP32(...) template int launch_pp32<__VA_ARGS__>(GemmArgs&, hipStream_t);
G4R_PP32(0, false, 256, 256, true, 0)    // 24 dense
G4R_PP32(1, false, 256, 256, true, 1)    // 24 conv
G4R_PP32(0, false, 192, 256, true, 0)    // 28
G4R_PP32(1, false, 192, 256, true, 0)
G4R_PP32(2, false, 256, 256, true, 1)    // all pyramid levels
G4R_PP32(0, false, 256, 256, false, 0)   // tile 34, operands of 2 GiB and more (tools: 30 dense)
G4R_PP32(1, false, 256, 256, false, 1)
G4R_PP32(2, false, 256, 256, false, 1)
#ifdef G4R_TOOLS_BUILD
G4R_PP32(0, false, 128, 384, true, 0)    // 27
G4R_PP32(1, false, 128, 384, true, 0)
G4R_PP32(0, true, 256, 256, true, 0)     // 25
G4R_PP32(1, true, 256, 256, true, 0)
G4R_PP32(1, false, 256, 256, false, 0)   // 30 conv
G4R_PP32(0, false, 256, 256, true, 1)    // 31 dense
G4R_PP32(1, false, 256, 256, true, 0)    // 33 conv
#endif
#undef G4R_PP32

}  // namespace G4R_GEMM_NS
