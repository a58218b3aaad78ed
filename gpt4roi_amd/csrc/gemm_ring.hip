// gemm_ring.hip -- the LDS-ring GEMM / implicit-GEMM kernel (gemm_bf16_nt_kernel): tiles 0, 4, 7, 13, 14 of launch_gemm's
// switch (gemm_bf16.hip) and, in the tools build, its superseded forms and A/B arms.
#include "gemm_common.h"

namespace {

// STAGES == 2: double buffer, one __syncthreads per K tile, latency hidden by 2-3 co-resident
//              workgroups per CU.
// STAGES >= 3: ring of LDS buffers, STAGES-1 tiles of LDS-DMA in flight, counted s_waitcnt vmcnt
//              (never 0 in steady state) + raw s_barrier, fragments double-buffered in registers;
//              one workgroup per CU owns most of the 160 KB LDS.
// BKT = K depth of one staged tile (64, or 32: half the LDS per stage -> more co-resident workgroups
// or a deeper ring at the same footprint).
template <int BM, int BN, int WM, int WN, int AMODE, bool GLDS, int STAGES, int BKT, int STYLE>
__global__ __launch_bounds__(WM* WN * 64, gemm_waves_per_eu(BM, BN, WM * WN, STAGES, BKT))
void gemm_bf16_nt_kernel(GemmArgs p) {
  constexpr int NW = WM * WN;
  constexpr int NT = NW * 64;
  constexpr int WTM = BM / WM, WTN = BN / WN;  // wave tile
  constexpr int TM = WTM / 32, TN = WTN / 32;  // 32x32 accumulators per wave
  constexpr int ROWB = BKT * 2;          // bytes per tile row
  constexpr int SPR = BKT / 8;           // 16-B slots per tile row
  constexpr int KK = BKT / 16;           // MFMA k-steps per tile
  constexpr int NA = BM * SPR / NT, NB = BN * SPR / NT;  // 16-B slots staged per thread
  constexpr int A_BYTES = BM * BKT * 2, B_BYTES = BN * BKT * 2;
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  static_assert(BM * SPR % NT == 0 && BN * SPR % NT == 0, "tile/threads mismatch");
  // bank-conflict swizzle of the 16-B slot index within a row (conflict-free ds_read_b128 lane groups)
  auto swz = [](int row) { return BKT == 64 ? ((row >> 1) & 7) : ((row >> 2) & 3); };
  static_assert(STAGES == 2 || GLDS, "the deep pipeline needs LDS-DMA staging");
  extern __shared__ __attribute__((aligned(16))) char smem[];  // STAGES * STAGE_BYTES

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  // ---- XCD-aware bijective remap of the 1-D grid (cdna_hip_programming.md 5.5 T1) ----
  const int nwg = p.tiles_m * p.tiles_n;
  int wg, split;
  g4r_workgroup_tile_slice(nwg, p.dbg == 11, wg, split);
  // Tile order = which operand the co-scheduled workgroups of one XCD share through its L2:
  //   M fastest: same W panel (weights are the big operand when M << N: LLaMA / ViT projections);
  //   N fastest: same A tile (activations are the big operand when M >> N: the implicit-GEMM convs,
  //              whose 9-tap gather was re-fetched once per column tile -- 2.5 GB/launch of fabric
  //              traffic at 192^2 against 170 MB algorithmic, profiles/r01_bench_rocprof.md).
  const int tile_m = p.n_fastest ? wg / p.tiles_n : wg % p.tiles_m;
  const int tile_n = p.n_fastest ? wg % p.tiles_n : wg / p.tiles_m;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int t_begin = split * p.tiles_per_split;
  int t_end = t_begin + p.tiles_per_split;
  const int nt_total = p.K / BKT;
  if (t_end > nt_total) t_end = nt_total;

  // ---- per-thread staging descriptors ----
  const h16_t* a_src[NA];
  int a_y[NA], a_x[NA];
  const h16_t* b_src[NB];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int pslot = (j * NW + wave) * 64 + lane;
    const int row = pslot / SPR, ps = pslot % SPR;
    const int kslot = ps ^ swz(row);
    int gm = m0 + row;
    if (gm > p.M - 1) gm = p.M - 1;
    if (AMODE == 0) {
      a_src[j] = p.A + (size_t)gm * p.lda + kslot * 8;
      a_y[j] = a_x[j] = 0;
    } else {
      const int hw = p.H * p.Wd;
      const int b = gm / hw, rem = gm - b * hw;
      a_y[j] = rem / p.Wd;
      a_x[j] = rem - a_y[j] * p.Wd;
      a_src[j] = p.A + (size_t)gm * p.lda + kslot * 8;  // centre tap of this pixel
    }
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int pslot = (j * NW + wave) * 64 + lane;
    const int row = pslot / SPR, ps = pslot % SPR;
    const int kslot = ps ^ swz(row);
    int gn = n0 + row;
    if (gn > p.N - 1) gn = p.N - 1;
    b_src[j] = p.W + (size_t)gn * p.ldw + kslot * 8;
  }

  auto stage = [&](int t, int buf) {
    char* sa = smem + buf * STAGE_BYTES;
    char* sb = sa + A_BYTES;
    int k0 = t * BKT;
    // A operand
    long a_off;
    int dy = 0, dx = 0;
    if (AMODE == 0) {
      a_off = k0;
    } else {
      // K tiles walk the taps FASTEST (channel slice outer): the nine shifted reads of one channel slice follow each
      // other within ~9 K tiles, so eight of them hit the L2 instead of HBM (the weights keep the [tap][Cin] layout)
      const int n_taps = 9 * p.groups;
      int ct = t / n_taps;
      int tap_lin = t - ct * n_taps;            // group * 9 + tap
      if (p.dbg == 7) {                         // A/B probe (tools only): taps outermost, the round-1 order
        const int per_tap = p.Cin / BKT;
        tap_lin = t / per_tap;
        ct = t - tap_lin * per_tap;
      }
      const int c0 = ct * BKT;
      const int grp = tap_lin / 9, tap = tap_lin - grp * 9;
      dy = tap / 3 - 1;
      dx = tap - (tap / 3) * 3 - 1;
      a_off = (long)grp * p.a_group_stride + ((long)dy * p.Wd + dx) * p.lda + c0;
      k0 = tap_lin * p.Cin + c0;
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      if (p.dbg == 3 && t != t_begin) break;  // ablation: A staged once, W keeps streaming
      const h16_t* src = a_src[j] + a_off;
      if (AMODE == 1) {
        const int yy = a_y[j] + dy, xx = a_x[j] + dx;
        if (yy < 0 || yy >= p.H || xx < 0 || xx >= p.Wd) src = p.zeros + (lane & 7) * 8;
      }
      char* dst_wave = sa + (j * NW + wave) * 1024;
      if (GLDS) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst_wave, 16, 0, 0);
      } else {
        *reinterpret_cast<uint4v*>(dst_wave + lane * 16) = *reinterpret_cast<const uint4v*>(src);
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (p.dbg == 5 && t != t_begin) break;  // ablation: W staged once, A keeps streaming
      const h16_t* src = b_src[j] + k0;
      char* dst_wave = sb + (j * NW + wave) * 1024;
      if (GLDS) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst_wave, 16, 0, 0);
      } else {
        *reinterpret_cast<uint4v*>(dst_wave + lane * 16) = *reinterpret_cast<const uint4v*>(src);
      }
    }
  };

  float16v acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment read offsets: row = base + (lane & 31), 16-B slot = (kk*2 + (lane>>5)) ^ ((row>>1)&7)
  const int frow = lane & 31;
  const int fsw = swz(frow);
  const int fhi = lane >> 5;
  const int a_row_off = (wm * WTM + frow) * ROWB;
  const int b_row_off = (wn * WTN + frow) * ROWB;

  auto compute = [&](int buf) {
    const char* sa = smem + buf * STAGE_BYTES;
    const char* sb = sa + A_BYTES;
    // STYLE 0: by LDS footprint (interleaved when >= 2 workgroups fit a CU), 1: interleaved, 2: burst
    if constexpr (STYLE == 1 || (STYLE == 0 && STAGES * (BM + BN) * BKT * 2 <= 80 * 1024)) {
      // 2-3 co-resident workgroups per CU: let the compiler interleave the 4 reads and 4 MFMAs of
      // each k-step (few VGPRs -> more waves).  Measured on MI355X: faster end to end than
      // issuing all 16 reads first (tools/gemm_ablate.py; DESIGN.md "GEMM experiments").
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int slot = ((kk * 2 + fhi) ^ fsw) << 4;
        h16x8 af[TM], wf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[i] = *reinterpret_cast<const h16x8*>(sa + a_row_off + i * 32 * ROWB + slot);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          wf[j] = *reinterpret_cast<const h16x8*>(sb + b_row_off + j * 32 * ROWB + slot);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = G4R_MFMA_32X32X16(wf[j], af[i], acc[i][j], 0, 0, 0);
      }
    } else if constexpr (STYLE == 3) {
      // every fragment read of the K tile goes out back to back and each k-step's MFMAs wait for THEIR reads only (counted
      // lgkmcnt).  The reads are inline asm: given plain loads the compiler orders them read, read, s_waitcnt lgkmcnt(0),
      // MFMA -- an LDS round trip in front of every k-step (the interleaved style above: ~150 cycles x KK per K tile against
      // 32 x KK of MFMA on a 64 x 64 tile) -- and the burst style below makes the first MFMA wait for ALL the reads.  Each
      // wait is tied ("+v") to the fragments it releases so that their MFMAs cannot move above it.
      h16x8 af[KK][TM], wf[KK][TN];
      const unsigned la = (unsigned)(size_t)(const __attribute__((address_space(3))) char*)(sa + a_row_off);
      const unsigned lb = (unsigned)(size_t)(const __attribute__((address_space(3))) char*)(sb + b_row_off);
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const unsigned slot = (unsigned)(((kk * 2 + fhi) ^ fsw) << 4);
#pragma unroll
        for (int i = 0; i < TM; ++i)
          asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[kk][i]) : "v"(la + slot), "n"(i * 32 * ROWB) : "memory");
#pragma unroll
        for (int j = 0; j < TN; ++j)
          asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(wf[kk][j]) : "v"(lb + slot), "n"(j * 32 * ROWB) : "memory");
      }
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(af[kk][0]) : "n"((TM + TN) * (KK - 1 - kk)));
#pragma unroll
        for (int i = 1; i < TM; ++i) asm volatile("" : "+v"(af[kk][i]));
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(wf[kk][j]));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = G4R_MFMA_32X32X16(wf[kk][j], af[kk][i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // one workgroup per CU: request every fragment of the K tile up front, then one MFMA burst
      h16x8 af[KK][TM], wf[KK][TN];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int slot = ((kk * 2 + fhi) ^ fsw) << 4;
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[kk][i] = *reinterpret_cast<const h16x8*>(sa + a_row_off + i * 32 * ROWB + slot);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          wf[kk][j] = *reinterpret_cast<const h16x8*>(sb + b_row_off + j * 32 * ROWB + slot);
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of the burst
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = G4R_MFMA_32X32X16(wf[kk][j], af[kk][i], acc[i][j], 0, 0, 0);
    }
  };

  if constexpr (STAGES == 2) {
    if (t_begin < t_end) {
      stage(t_begin, 0);
      __syncthreads();  // drains the LDS-DMA queue (vmcnt(0)) and publishes the tile
      int cur = 0;
      for (int t = t_begin; t < t_end - 1; ++t) {
        if (p.dbg != 1) stage(t + 1, cur ^ 1);
        if (p.dbg != 2) compute(cur);
        __syncthreads();
        cur ^= 1;
      }
      compute(cur);
    }
  } else {
    constexpr int NLD = NA + NB;  // LDS-DMA instructions per thread per tile
    const int nt = t_end - t_begin;
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
      if (s < nt) stage(t_begin + s, s);
    int rd = 0, wr = STAGES - 1;
    for (int i = 0; i < nt; ++i) {
      // tile i must have landed; up to STAGES-2 younger tiles stay in flight across the barrier
      const int ahead = nt - 1 - i;
      if (STAGES >= 4 && ahead >= 2)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NLD) : "memory");
      else if (ahead >= 1)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // everyone's tile i is in LDS; everyone is done reading tile i-1
      asm volatile("" ::: "memory");
      if (i + STAGES - 1 < nt && p.dbg != 1) stage(t_begin + i + STAGES - 1, wr);
      if (p.dbg != 2 || i + 1 == nt) compute(rd);
      rd = rd + 1 == STAGES ? 0 : rd + 1;
      wr = wr + 1 == STAGES ? 0 : wr + 1;
    }
  }

  // ---- epilogue through LDS (row-major, whole-line stores: see gemm_epilogue_lds), 32 rows per pass ----
  __syncthreads();   // every wave has read its last fragments: the staging buffers are free
  gemm_epilogue_lds<TM, TN, 32>(p, acc, smem + wave * EpiLds<TN, 32>::WAVE_BYTES, m0 + wm * WTM, n0 + wn * WTN, lane, split);
}

}  // namespace

G4R_GEMM_NS_OPEN

template <int BM, int BN, int WM, int WN, int AMODE, bool GLDS, int STAGES, int BKT, int STYLE>
int launch_tile(GemmArgs& p, hipStream_t stream) {
  gemm_split_geometry(p, BKT);
  p.tiles_m = g4r_ceil_div(p.M, BM);
  p.tiles_n = g4r_ceil_div(p.N, BN);
  const size_t ring = (size_t)STAGES * (BM + BN) * BKT * 2, epi = (size_t)WM * WN * EpiLds<BN / WN / 32, 32>::WAVE_BYTES;
  const size_t lds = ring > epi ? ring : epi;
  auto kern = gemm_bf16_nt_kernel<BM, BN, WM, WN, AMODE, GLDS, STAGES, BKT, STYLE>;
  static G4rPerDeviceOnce attr_set;
  if (int rc = gemm_raise_lds_limit(attr_set, reinterpret_cast<const void*>(kern), lds, "gemm: hipFuncSetAttribute")) return rc;
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n, p.splits), dim3(WM * WN * 64), lds, stream, p);
  G4R_CHECK_LAUNCH("gemm_bf16_nt");
  return gemm_reduce_tail(p, stream);
}

// the forms launch_gemm's switch names (tile id behind each), dense (AMODE 0) and convolution (AMODE 1)
#define G4R_RING_TILE(BM, BN, WM, WN, ...)                                                  \
  template int launch_tile<BM, BN, WM, WN, 0, __VA_ARGS__>(GemmArgs&, hipStream_t);         \
  template int launch_tile<BM, BN, WM, WN, 1, __VA_ARGS__>(GemmArgs&, hipStream_t);
G4R_RING_TILE(128, 128, 2, 2, true, 2, 64, 0)   // 0
G4R_RING_TILE(64, 128, 1, 4, true, 2, 64, 0)    // 4
G4R_RING_TILE(128, 128, 2, 4, true, 4, 64, 3)   // 7
G4R_RING_TILE(64, 128, 1, 4, true, 3, 64, 3)    // 13
G4R_RING_TILE(64, 64, 2, 2, true, 4, 64, 3)     // 14
#ifdef G4R_TOOLS_BUILD
G4R_RING_TILE(256, 128, 4, 2, true, 2, 64, 0)   // 1
G4R_RING_TILE(128, 128, 2, 2, false, 2, 64, 0)  // 2
G4R_RING_TILE(128, 128, 2, 2, true, 3, 64, 0)   // 5
G4R_RING_TILE(128, 128, 2, 2, true, 4, 64, 0)   // 6
G4R_RING_TILE(256, 128, 4, 2, true, 3, 64, 0)   // 8
G4R_RING_TILE(256, 256, 2, 4, true, 2, 64, 0)   // 9
G4R_RING_TILE(128, 128, 2, 4, true, 2, 64, 0)   // 10
G4R_RING_TILE(128, 64, 2, 2, true, 2, 64, 0)    // 11
G4R_RING_TILE(64, 128, 1, 4, true, 4, 64, 0)    // 12
G4R_RING_TILE(128, 64, 2, 2, true, 4, 64, 0)    // 15
template int launch_tile<128, 128, 2, 2, 0, true, 2, 64, 3>(GemmArgs&, hipStream_t);   // 40 (dense only, as 43 / 44 / 47)
template int launch_tile<64, 128, 1, 4, 0, true, 3, 64, 0>(GemmArgs&, hipStream_t);
template int launch_tile<64, 64, 2, 2, 0, true, 4, 64, 0>(GemmArgs&, hipStream_t);
template int launch_tile<128, 128, 2, 4, 0, true, 4, 64, 0>(GemmArgs&, hipStream_t);
#endif
#undef G4R_RING_TILE

}  // namespace G4R_GEMM_NS
