// gemm_bf16.hip -- bf16 MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950 (CDNA4).
//
//   C[M,N] = epilogue( A[M,K] . W[N,K]^T )          (nn.Linear layout: W is [out, in])
//
// One kernel template serves every dense contraction of the region-feature path
// (SURVEY.md section 8a rows a4, a7, a8, a14, a16 -- the arithmetic the reference delegates to
// cuBLAS/cuDNN through torch.nn.Linear / nn.Conv2d, e.g. gpt4roi/models/layers.py:129-144,
// 257-270 and llava/model/llava.py:52):
//   AMODE 0  dense A [M, lda]
//   AMODE 1  implicit GEMM of a 3x3 / pad 1 / stride 1 convolution over NHWC activations:
//            row m = pixel (b, y, x), K index = ((group * 9 + tap) * Cin + c), walked taps-fastest;
//            out-of-image taps read a zero line.  `groups` > 1 sums several convolutions in one accumulator
//            (the "sum_l pconv_l(roi_feats[l])" of layers.py:321-324).
//
// Machine mapping (MI355X_MICROARCH.md / cdna_hip_programming.md section 5):
//   * v_mfma_f32_32x32x16_bf16, operands swapped (W as the "A" operand) so that a lane's 4
//     consecutive accumulator registers are 4 consecutive N columns -> 8/16-byte stores;
//   * BK = 64; tiles staged global->LDS with global_load_lds_dwordx4 (LDS-DMA, no VGPR round
//     trip), double buffered, one barrier per K tile;
//   * the LDS image is lane-linear for the DMA, so the bank-conflict swizzle
//     (16-B slot ^= (row>>1)&7) is applied on the per-lane SOURCE address and again on the
//     ds_read_b128 address (rule "both sides or neither");
//   * XCD-aware, bijective workgroup -> tile map so neighbouring tiles share panels in one L2.
//
// This file holds the C entry points, the tile switch (launch_gemm) and the two small kernels every family shares; the kernel
// families live in gemm_ring.hip, gemm_pp32.hip, gemm_w4k64.hip, gemm_w4k64p.hip and gemv_bf16.hip (gemm_common.h; DESIGN.md
// "GEMM source map").
#include "gemm_common.h"

int G4R_GEMM_NS::g_gemm_dbg = 0;

namespace {

// split-K combine + epilogue: C = act(sum_s ws[s] + bias) + residual
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmArgs p) {
  const long total = (long)p.M * p.N;
  // vector path: 4 consecutive columns per thread, 16-byte loads of every partial (the scalar loops below moved 4 bytes per
  // lane per load: 10 us average over the 89 reduce launches of a round-2 step).  Same summation order (s = 0, 1, ...) and
  // the same bias -> activation -> residual -> one rounding sequence: bit-identical to the scalar path.
  // (base pointers too: gemm() passes column-sliced views of C / residual / bias -- 16-byte loads of the bias and 8/16-byte
  // accesses of C and the residual need the slice itself aligned, not only its leading dimension)
  const bool ptrs_aligned = ((uintptr_t)p.C & 15) == 0 && ((uintptr_t)p.residual & 7) == 0 && ((uintptr_t)p.bias & 15) == 0 &&
                            ((uintptr_t)p.ws & 15) == 0;
  if (ptrs_aligned && (p.N & 3) == 0 && (p.ldc & 3) == 0 && (p.ldr & 3) == 0 && (p.act != 4 || (p.ldc & 1) == 0)) {
    const int n4 = p.N >> 2;
    const long quads = (long)p.M * n4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
      const int c4 = (int)(i % n4) * 4;
      const long m = i / n4;
      float4v x = {0.f, 0.f, 0.f, 0.f};
      const float* src = p.ws + m * p.N + c4;
      for (int s0 = 0; s0 < p.splits; s0 += 4) {      // up to 4 partial loads in flight
        float4v v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (s0 + u < p.splits) v[u] = *reinterpret_cast<const float4v*>(src + (size_t)(s0 + u) * total);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (s0 + u < p.splits) x += v[u];
      }
      if (p.act == 4) {
        const float s0v = h16lo(pack_h16x2(x[0] / (1.f + __expf(-x[0])), 0.f));
        const float s1v = h16lo(pack_h16x2(x[2] / (1.f + __expf(-x[2])), 0.f));
        *reinterpret_cast<uint32_t*>(reinterpret_cast<h16_t*>(p.C) + (size_t)m * p.ldc + (c4 >> 1)) =
            pack_h16x2(s0v * x[1], s1v * x[3]);
        continue;
      }
      if (p.bias) {
        const float4v bv = *reinterpret_cast<const float4v*>(p.bias + c4);
        x += bv;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = apply_act(x[e], p.act);
      if (p.residual) {
        const uint2v r = *reinterpret_cast<const uint2v*>(p.residual + (size_t)m * p.ldr + c4);
        x[0] += h16lo(r.x); x[1] += h16hi(r.x); x[2] += h16lo(r.y); x[3] += h16hi(r.y);
      }
      if (p.out_f32) {
        *reinterpret_cast<float4v*>(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + c4) = x;
      } else {
        const uint2v w = {pack_h16x2(x[0], x[1]), pack_h16x2(x[2], x[3])};
        *reinterpret_cast<uint2v*>(reinterpret_cast<h16_t*>(p.C) + (size_t)m * p.ldc + c4) = w;
      }
    }
    return;
  }
  if (p.act == 4) {  // SwiGLU over interleaved (gate, up) column pairs: C has N/2 columns (bf16)
    const int half = p.N >> 1;
    const long pairs = (long)p.M * half;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (long)gridDim.x * 256) {
      const int c = (int)(i % half);
      const long m = i / half;
      float g = 0.f, u = 0.f;
      for (int s = 0; s < p.splits; ++s) {
        const float2 v = *reinterpret_cast<const float2*>(p.ws + (size_t)s * total + m * p.N + 2 * c);
        g += v.x;
        u += v.y;
      }
      const float sg = h16lo(pack_h16x2(g / (1.f + __expf(-g)), 0.f));
      reinterpret_cast<h16_t*>(p.C)[(size_t)m * p.ldc + c] = f32_to_h16(sg * u);
    }
    return;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i % p.N);
    const long m = i / p.N;
    float x = 0.f;
    for (int s = 0; s < p.splits; ++s) x += p.ws[(size_t)s * total + i];
    if (p.bias) x += p.bias[n];
    x = apply_act(x, p.act);
    if (p.residual) x += h16_to_f32(p.residual[(size_t)m * p.ldr + n]);
    if (p.out_f32)
      reinterpret_cast<float*>(p.C)[(size_t)m * p.ldc + n] = x;
    else
      reinterpret_cast<h16_t*>(p.C)[(size_t)m * p.ldc + n] = f32_to_h16(x);
  }
}

// Tiny/irregular contractions (K not a multiple of 64, e.g. the Linear(4,256) of pos_embedd,
// gpt4roi/models/layers.py:260-267): one thread per output, fp32 accumulate.  Not a hot path.
__global__ __launch_bounds__(256) void small_linear_kernel(const h16_t* __restrict__ A,
                                                           const h16_t* __restrict__ W,
                                                           const float* __restrict__ bias,
                                                           void* __restrict__ C, int M, int N, int K,
                                                           int lda, int ldw, int ldc, int act,
                                                           int out_f32) {
  const long total = (long)M * N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i % N);
    const long m = i / N;
    float x = 0.f;
    for (int k = 0; k < K; ++k) x += h16_to_f32(A[m * lda + k]) * h16_to_f32(W[(size_t)n * ldw + k]);
    if (bias) x += bias[n];
    x = apply_act(x, act);
    if (out_f32)
      reinterpret_cast<float*>(C)[m * ldc + n] = x;
    else
      reinterpret_cast<h16_t*>(C)[m * ldc + n] = f32_to_h16(x);
  }
}

}  // namespace

int G4R_GEMM_NS::gemm_reduce_tail(GemmArgs& p, hipStream_t stream) {
  if (p.splits <= 1 || p.defer_reduce) return G4R_OK;
  long total = (long)p.M * p.N;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, stream, p);
  G4R_CHECK_LAUNCH("splitk_reduce");
  return G4R_OK;
}

namespace {

// K tile of the kernel a tile id launches: 32 for the ring ping-pong tiles (launch_pp32), 64 for the rest
constexpr int gemm_tile_bk(int tile_cfg) {
  switch (tile_cfg) {
    case 24: case 25: case 27: case 28: case 30: case 31: case 33: return 32;
    default: return BK;
  }
}

template <int AMODE>
int launch_gemm(GemmArgs& p, int tile_cfg, hipStream_t stream) {
  if (g_gemm_dbg == 9) p.n_fastest = 0;     // tools: force the tile order (A/B of the L2 sharing pattern)
  if (g_gemm_dbg == 10) p.n_fastest = 1;
  // grouped tile order for dense launches with many row tiles (ring ping-pong kernel): tools modes 31 / 32 / 33 force a group of
  // 8 / 4 / 16 row tiles, 30 forces the plain order
  p.group_m = 0;
  if (AMODE == 0 && (tile_cfg == 24 || tile_cfg == 28 || tile_cfg == 34 || tile_cfg == 35 || tile_cfg == 36)) {
    const int tm = g4r_ceil_div(p.M, tile_cfg == 28 ? 192 : 256);
    if (tm >= 12) p.group_m = 8;
    if (g_gemm_dbg == 30) p.group_m = 0;
    if (g_gemm_dbg == 31) p.group_m = 8;
    if (g_gemm_dbg == 32) p.group_m = 4;
    if (g_gemm_dbg == 33) p.group_m = 16;
  }
  if (AMODE >= 1 && g_gemm_dbg == 41) p.group_m = -2;   // tools: conv, an XCD's wave = 16 pixel tiles x 2 weight panels
  if (AMODE >= 1 && g_gemm_dbg == 42) p.group_m = -1;   // tools: 32 pixel tiles x 1 weight panel
  switch (tile_cfg) {
    // ---- the tiles kernels.py dispatches (pick_tile / pick_conv_tile / long_k_plan / partial_wave_plan / layers.py) ----
    case 0: return launch_tile<128, 128, 2, 2, AMODE, true>(p, stream);
    case 4: return launch_tile<64, 128, 1, 4, AMODE, true>(p, stream);
    case 7: return launch_tile<128, 128, 2, 4, AMODE, true, 4, 64, 3>(p, stream);   // 8 waves, 64x32 wave tiles; counted-wait fragment pipeline
    // Small-M shapes (CLIP ViT, M = 577; K = 1024 is only 16 K tiles): fewer workgroups than CUs, so what matters is ONE
    // workgroup's latency -> deep LDS-DMA rings instead of co-resident workgroups.
    case 13: return launch_tile<64, 128, 1, 4, AMODE, true, 3, 64, 3>(p, stream);   // 72 KB ring of 3: 2 wg/CU; counted-wait fragment pipeline
    case 14: return launch_tile<64, 64, 2, 2, AMODE, true, 4, 64, 3>(p, stream);    // 64 KB ring of 4: 2 wg/CU; counted-wait fragment pipeline
    case 34: return launch_w4k64<AMODE>(p, stream);                              // 256x256, 4 waves x (128x128), K 64 x 2 buffers refilled as consumed (round 5)
    case 36: p.persist_any_k = 1; return launch_w4k64<AMODE>(p, stream);         // tile 34 with its persistent form offered at every K (round 6; tests)
    case 24:                                                                     // 256x256 ping-pong, K 32 ring of 4 (G4R_BIG_TILE=24; operands >= 2 GiB)
      // the implicit-GEMM convs take the rotated single-barrier schedule (192^2 conv 693 -> 668 us, tools/gemm_bench.cpp
      // tile 31); the dense GEMMs lose 8-12 % on it (4096^3 1172 -> 1076 TF/s) and keep the two-barrier form
      if constexpr (AMODE >= 1) return launch_pp32<AMODE, false, 256, 256, true, 1>(p, stream);
      else return launch_pp32<AMODE>(p, stream);
    case 28: return launch_pp32<AMODE, false, 192, 256>(p, stream);              // 192x256 ring ping-pong (767 x 12288: 4 x 48 = 192 workgroups)
#ifdef G4R_TOOLS_BUILD
    // ---- superseded forms and A/B arms: compiled only into the tools build (G4R_EXTRA_HIPCC_FLAGS=-DG4R_TOOLS_BUILD python -m
    //      gpt4roi_amd.build --force); the shipped library holds the dispatched kernels only ----
    case 1: return launch_tile<256, 128, 4, 2, AMODE, true>(p, stream);
    case 2: return launch_tile<128, 128, 2, 2, AMODE, false>(p, stream);  // register-staged A/B probe
    case 5: return launch_tile<128, 128, 2, 2, AMODE, true, 3>(p, stream);   // 96 KB ring
    case 6: return launch_tile<128, 128, 2, 2, AMODE, true, 4>(p, stream);   // 128 KB ring
    case 8: return launch_tile<256, 128, 4, 2, AMODE, true, 3>(p, stream);   // 144 KB ring, 8 waves
    case 9: return launch_tile<256, 256, 2, 4, AMODE, true, 2>(p, stream);   // 128 KB, wave tile 128x64
    case 10: return launch_tile<128, 128, 2, 4, AMODE, true, 2>(p, stream);  // 8 waves x (64x32), 2 wg/CU
    case 11: return launch_tile<128, 64, 2, 2, AMODE, true, 2>(p, stream);   // 48 KB: 3 wg/CU
    // (12-21 of round 1 were the BK = 32 / interleaved-read ring experiments of DESIGN.md section 3; they lost and
    // were removed.)
    case 12: return launch_tile<64, 128, 1, 4, AMODE, true, 4>(p, stream);   // 96 KB ring of 4
    case 15: return launch_tile<128, 64, 2, 2, AMODE, true, 4>(p, stream);   // 96 KB ring of 4
    // A/B arms of round 3c (dense GEMM only): tiles 13 / 14 / 7 with the compiler's own read order (STYLE 0; the counted-wait
    // fragment pipeline, STYLE 3, is their production form: ViT qkv 10.9 -> 10.8 us, o 8.2 -> 7.9, fc1 15.5 -> 14.6, fc2 21.1 ->
    // 20.4, LLaMA o_proj 41.7 -> 40.2), and the two-stage 128 x 128 tile WITH the pipeline (no gain: 68.3 vs 69.6 us)
    case 40: if constexpr (AMODE == 0) return launch_tile<128, 128, 2, 2, AMODE, true, 2, 64, 3>(p, stream); else break;
    case 43: if constexpr (AMODE == 0) return launch_tile<64, 128, 1, 4, AMODE, true, 3>(p, stream); else break;
    case 44: if constexpr (AMODE == 0) return launch_tile<64, 64, 2, 2, AMODE, true, 4>(p, stream); else break;
    case 47: if constexpr (AMODE == 0) return launch_tile<128, 128, 2, 4, AMODE, true, 4>(p, stream); else break;
    case 35: if constexpr (AMODE == 0) return launch_w4k64<AMODE, true>(p, stream); else break;   // tile 34 + s_memtime stamps
    case 27: return launch_pp32<AMODE, false, 128, 384>(p, stream);              // 128x384 ring ping-pong (767 x 12288: 192 workgroups)
    case 25: return launch_pp32<AMODE, true>(p, stream);                         // tile 24 + s_memtime stamps
    case 30: return launch_pp32<AMODE, false, 256, 256, false>(p, stream);       // A/B arm: pieces by global_load_lds (the round-2 form)
    case 31: return launch_pp32<AMODE, false, 256, 256, true, 1>(p, stream);     // rotated single-barrier schedule (A/B arm for dense)
    case 33: return launch_pp32<AMODE, false, 256, 256, true, 0>(p, stream);     // two-barrier schedule (A/B arm for the convs)
#endif
    default: break;
  }
  return g4r_note_error(G4R_ERR_INVALID_ARG, "gemm: unknown tile_cfg (superseded forms / A-B arms exist in the tools build only: -DG4R_TOOLS_BUILD)");
}
}  // namespace


extern "C" {

// tools/ only: ablation switch for the GEMM main loop (0 = normal).  Not declared in include/.
//   1 / 2: skip the staging / the compute of the generic kernel's loop;  7: taps-outermost K order of the conv (A/B arm);
//   8: pieces by global_load_lds instead of buffer loads;  9 / 10: force the M-fastest / N-fastest tile order;
//   11: the round-2 workgroup -> tile map (tiles only, every XCD sees all K slices);  100 + v: GEMV variant v.
#ifndef G4R_F16
void g4r_gemm_debug_mode(int mode) { g_gemm_dbg = mode; }
#endif

// See include/g4r_kernels.h for the contract.
// C = A W^T as `*splits_out` fp32 K-slice partials [slice][M][N] in `workspace` (>= splits * M * N floats), WITHOUT the reduce
// launch: the consumer combines them (g4r_rmsnorm_splitk_bf16: the reduce of the LLaMA down_proj folded into the next
// RMSNorm).  splits >= 2; the number of slices actually written (<= splits) is returned through splits_out.
int g4r_gemm_bf16_nt_partials(const void* A, const void* W, float* workspace, int M, int N, int K, int lda, int ldw,
                              int splits, int tile_cfg, int* splits_out, void* stream) {
  G4R_REQUIRE(M > 0 && N > 0 && K > 0 && K % BK == 0, "gemm_partials: K must be a positive multiple of 64");
  G4R_REQUIRE(A && W && workspace && splits_out, "gemm_partials: null pointer");
  G4R_REQUIRE((lda % 8) == 0 && (ldw % 8) == 0 && splits >= 2, "gemm_partials: 16-byte rows, splits >= 2");
  {
    // the slices the tile will really cut, checked BEFORE the launch: a tile that clamps to one slice would run its normal
    // epilogue into `workspace`
    GemmArgs q = {};
    q.K = K; q.splits = splits;
    gemm_split_geometry(q, gemm_tile_bk(tile_cfg));
    G4R_REQUIRE(q.splits >= 2, "gemm_partials: the tile's K slices collapse to one (K too short for `splits`)");
  }
  GemmArgs p = {};
  p.A = (const h16_t*)A; p.W = (const h16_t*)W; p.C = workspace; p.ws = workspace;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = N; p.ldr = 0;
  p.act = 0; p.out_f32 = 1; p.dbg = g_gemm_dbg;
  p.n_fastest = (long)M * 1 > (long)N * 2;
  p.splits = splits;
  p.defer_reduce = 1;
  const int rc = launch_gemm<0>(p, tile_cfg, (hipStream_t)stream);
  *splits_out = p.splits;
  G4R_REQUIRE(rc != G4R_OK || p.splits >= 2, "gemm_partials: the tile's K slices collapsed to one (K too short for `splits`)");
  return rc;
}

// The fused q|k|v projection of a LLaMA layer with RoPE and the KV-cache append in the GEMM epilogue: A [B*T, K] hidden rows,
// W [3*heads*128, K] (q | k | v rows).  q_out [B*T, heads*128] receives the rotated queries; k_cache / v_cache (this layer's
// cache, rows `cache_row` elements apart, sequences `cache_batch` apart) receive the rotated keys / the values at rows
// pos0 + t.  cos / sin: [max_pos][64] fp32.  Same arithmetic and rounding points as g4r_gemm_bf16_nt + g4r_rope_qkv_bf16
// (the projection is rounded to bf16, rotated in fp32, rounded once more).  tile_cfg: 24 or 28 (0 = 28).
int g4r_gemm_qkv_rope_bf16(const void* A, const void* W, int B, int T, int K, int lda, int ldw, int heads, int head_dim,
                           void* q_out, void* k_cache, void* v_cache, long cache_row, long cache_batch,
                           const float* cos_tab, const float* sin_tab, int pos0, int tile_cfg, void* stream) {
  G4R_REQUIRE(B > 0 && T > 0 && K > 0 && K % BK == 0 && heads > 0, "gemm_qkv_rope: bad shape");
  G4R_REQUIRE(head_dim == 128 && (heads * head_dim) % 256 == 0, "gemm_qkv_rope: head_dim 128, heads * 128 a multiple of 256");
  G4R_REQUIRE(A && W && q_out && k_cache && v_cache && cos_tab && sin_tab, "gemm_qkv_rope: null pointer");
  G4R_REQUIRE((lda % 8) == 0 && (ldw % 8) == 0 && (cache_row % 8) == 0 && (cache_batch % 8) == 0, "gemm_qkv_rope: 16-byte rows");
  if (tile_cfg == 0) tile_cfg = 28;
  G4R_REQUIRE(tile_cfg == 24 || tile_cfg == 28 || tile_cfg == 34 || tile_cfg == 36, "gemm_qkv_rope: 256-wide tiles only (24 / 28 / 34 / 36)");
  GemmArgs p = {};
  p.A = (const h16_t*)A; p.W = (const h16_t*)W; p.C = q_out;
  p.M = B * T; p.N = 3 * heads * head_dim; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = heads * head_dim;
  p.act = 5; p.dbg = g_gemm_dbg;
  p.n_fastest = 0;
  p.splits = 1;
  p.rope_q = (h16_t*)q_out; p.rope_k = (h16_t*)k_cache; p.rope_v = (h16_t*)v_cache;
  p.rope_cos = cos_tab; p.rope_sin = sin_tab; p.rope_krow = cache_row; p.rope_kbatch = cache_batch;
  p.rope_T = T; p.rope_pos0 = pos0; p.rope_HD = heads * head_dim;
  return launch_gemm<0>(p, tile_cfg, (hipStream_t)stream);
}

int g4r_gemm_bf16_nt(const void* A, const void* W, void* C, const float* bias, const void* residual,
                     float* workspace, int M, int N, int K, int lda, int ldw, int ldc, int ldr,
                     int act, int out_f32, int splits, int tile_cfg, void* stream) {
  G4R_REQUIRE(M >= 0 && N >= 0 && K >= 0, "gemm: negative shape");
  if (M == 0 || N == 0) return G4R_OK;
  G4R_REQUIRE(A && W && C, "gemm: null pointer");
  G4R_REQUIRE(act >= 0 && act <= 4, "gemm: act must be 0..4 (5 = the fused RoPE epilogue: g4r_gemm_qkv_rope_bf16)");
  G4R_REQUIRE(act != 4 || (N % 4 == 0 && ldc % 2 == 0 && !residual && !bias && !out_f32 && K % BK == 0),
              "gemm: swiglu epilogue needs N % 4 == 0, bf16 output, no bias/residual");
  if (M == 1 && K % 8 == 0 && (ldw % 8) == 0 && splits == 1 && K >= 512 && K <= G4R_GEMV_MAX_K && (act != 4 || N % 4 == 0)) {
    // single-token decode: weight-streaming GEMV
    gemv_dispatch(g_gemm_dbg >= 100 ? g_gemm_dbg - 100 : -1, 0, (const h16_t*)A, nullptr, 0.f, 0, 0, (const h16_t*)W, C,
                  bias, (const h16_t*)residual, N, K, ldw, act, out_f32, (hipStream_t)stream);
    G4R_CHECK_LAUNCH("gemv_bf16");
    return G4R_OK;
  }
  if (K % BK != 0 || K == 0) {
    G4R_REQUIRE(residual == nullptr, "gemm: residual unsupported on the small-K path");
    long total = (long)M * N;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(small_linear_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const h16_t*)A, (const h16_t*)W, bias, C, M, N, K, lda, ldw, ldc, act, out_f32);
    G4R_CHECK_LAUNCH("small_linear");
    return G4R_OK;
  }
  G4R_REQUIRE((lda % 8) == 0 && (ldw % 8) == 0, "gemm: lda/ldw must be multiples of 8 (16-byte rows)");
  G4R_REQUIRE(splits >= 1, "gemm: splits >= 1");
  G4R_REQUIRE(splits == 1 || workspace, "gemm: split-K needs a workspace of splits*M*N floats");
  GemmArgs p = {};
  p.A = (const h16_t*)A; p.W = (const h16_t*)W; p.C = C; p.ws = workspace; p.bias = bias;
  p.residual = (const h16_t*)residual;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldr = ldr;
  p.act = act; p.out_f32 = out_f32; p.dbg = g_gemm_dbg;
  p.n_fastest = (long)M * 1 > (long)N * 2;
  p.splits = splits;
  return launch_gemm<0>(p, tile_cfg, (hipStream_t)stream);
}

// y [N] = act(W [N, K] . rmsnorm(x; gamma, eps) + bias) + residual for ONE activation row: the projections of the decode
// step with the RMSNorm in front of them fused in (gamma null = no norm).  See g4r_kernels.h.
int g4r_gemv_rmsnorm_bf16(const void* x, const float* gamma, float eps, const void* W, void* C, const float* bias,
                          const void* residual, int N, int K, int ldw, int act, int out_f32, void* stream) {
  G4R_REQUIRE(N > 0 && K >= 512 && K % 8 == 0 && ldw % 8 == 0 && ldw >= K, "gemv: K >= 512, K and ldw multiples of 8");
  G4R_REQUIRE(x && W && C, "gemv: null pointer");
  G4R_REQUIRE(act >= 0 && act <= 4, "gemv: act must be 0..4");
  G4R_REQUIRE(act != 4 || (N % 4 == 0 && !residual && !bias && !out_f32), "gemv: swiglu needs N % 4 == 0, bf16 output");
  G4R_REQUIRE(K <= (gamma ? 8192 : G4R_GEMV_MAX_K), "gemv: K <= 8192 with the fused norm, <= 32736 without (x is staged in 64 KB of LDS)");
  gemv_dispatch(g_gemm_dbg >= 100 ? g_gemm_dbg - 100 : -1, gamma ? 1 : 0, (const h16_t*)x, gamma, eps, 0, 0,
                (const h16_t*)W, C, bias, (const h16_t*)residual, N, K, ldw, act, out_f32, (hipStream_t)stream);
  G4R_CHECK_LAUNCH("gemv_rmsnorm_bf16");
  return G4R_OK;
}

// C [N] = W [N, K] . a + bias + residual, where a [K = H * head_dim] is the decode-attention output assembled on the fly
// from the per-split partials g4r_attn_decode_bf16 wrote with defer_merge (partials [H][splits][head_dim + 2] fp32).
int g4r_gemv_attn_merge_bf16(const float* partials, int splits, int head_dim, const void* W, void* C, const float* bias,
                             const void* residual, int N, int K, int ldw, int out_f32, void* stream) {
  G4R_REQUIRE(N > 0 && K >= 512 && K % 8 == 0 && ldw % 8 == 0 && ldw >= K && K <= G4R_GEMV_MAX_K, "gemv_attn_merge: bad shape");
  G4R_REQUIRE(partials && W && C, "gemv_attn_merge: null pointer");
  G4R_REQUIRE(splits >= 1 && splits <= 64 && (head_dim == 64 || head_dim == 128) && K % head_dim == 0,
              "gemv_attn_merge: splits in [1, 64], head_dim 64 or 128 dividing K");
  gemv_dispatch(-1, 2, nullptr, partials, 0.f, splits, head_dim, (const h16_t*)W, C, bias, (const h16_t*)residual, N, K,
                ldw, 0, out_f32, (hipStream_t)stream);
  G4R_CHECK_LAUNCH("gemv_attn_merge_bf16");
  return G4R_OK;
}

int g4r_conv3x3_nhwc_bf16(const void* X, const void* W, void* Y, const float* bias, const void* zeros,
                          float* workspace, int batch, int H, int Wd, int Cin, int Cout, int groups,
                          long x_group_stride, int act, int out_f32, int splits, int tile_cfg,
                          void* stream) {
  G4R_REQUIRE(batch >= 0 && H > 0 && Wd > 0 && Cin > 0 && Cout > 0 && groups >= 1, "conv3x3: bad shape");
  if (batch == 0) return G4R_OK;
  G4R_REQUIRE(X && W && Y && zeros, "conv3x3: null pointer");
  G4R_REQUIRE((Cin % BK) == 0, "conv3x3: Cin must be a multiple of 64");
  G4R_REQUIRE(act >= 0 && act <= 3, "conv3x3: act must be 0..3");
  G4R_REQUIRE(splits >= 1 && (splits == 1 || workspace), "conv3x3: split-K needs a workspace");
  GemmArgs p = {};
  p.A = (const h16_t*)X; p.W = (const h16_t*)W; p.C = Y; p.ws = workspace; p.bias = bias;
  p.zeros = (const h16_t*)zeros;
  p.M = batch * H * Wd; p.N = Cout; p.K = groups * 9 * Cin;
  p.lda = Cin; p.ldw = p.K; p.ldc = Cout; p.ldr = 0;
  p.act = act; p.out_f32 = out_f32;
  p.H = H; p.Wd = Wd; p.Cin = Cin; p.groups = groups; p.a_group_stride = x_group_stride;
  p.n_fastest = 1; p.dbg = g_gemm_dbg;
  p.splits = splits;
  return launch_gemm<1>(p, tile_cfg, (hipStream_t)stream);
}

// The 3x3 convolutions of ONE fuse round over all pyramid levels as a single implicit GEMM (gpt4roi/models/layers.py:218-236
// applies the SAME ConvModule to every level): X / Y hold the levels' NHWC maps stacked [level][b][y][x][C]; row m decodes
// to (level, b, y, x) and shifts inside its own map.  For the 336^2 pyramid (192^2 + 96^2 + 48^2 + 24^2 = 48960 rows) the
// launch has 192 x 4 = 768 tiles of 256 x 256 = exactly three waves of the 256 CUs, where the four separate launches leave
// the chip partly idle in each of their tails (and the two small maps latency-bound on split-K tiles).
int g4r_conv3x3_mlvl_nhwc_bf16(const void* X, const void* W, void* Y, const float* bias, const void* zeros, int n_levels,
                               const int* level_h, const int* level_w, int batch, int Cin, int Cout, int act,
                               void* stream) {
  G4R_REQUIRE(n_levels >= 1 && n_levels <= 4 && batch >= 1 && Cin > 0 && Cout > 0, "conv3x3_mlvl: 1..4 levels");
  G4R_REQUIRE(X && W && Y && zeros && level_h && level_w, "conv3x3_mlvl: null pointer");
  G4R_REQUIRE((Cin % BK) == 0, "conv3x3_mlvl: Cin must be a multiple of 64");
  G4R_REQUIRE(act >= 0 && act <= 3, "conv3x3_mlvl: act must be 0..3");
  GemmArgs p = {};
  long rows = 0;
  for (int l = 0; l < n_levels; ++l) {
    G4R_REQUIRE(level_h[l] > 0 && level_w[l] > 0, "conv3x3_mlvl: bad map size");
    p.lvl_start[l] = (int)rows;
    p.lvl_h[l] = level_h[l]; p.lvl_w[l] = level_w[l];
    rows += (long)batch * level_h[l] * level_w[l];
  }
  G4R_REQUIRE(rows < (1L << 31), "conv3x3_mlvl: too many rows");
  for (int l = n_levels; l <= 4; ++l) p.lvl_start[l] = (int)rows;
  p.n_lvl = n_levels;
  p.A = (const h16_t*)X; p.W = (const h16_t*)W; p.C = Y; p.bias = bias; p.zeros = (const h16_t*)zeros;
  p.M = (int)rows; p.N = Cout; p.K = 9 * Cin;
  p.lda = Cin; p.ldw = p.K; p.ldc = Cout;
  p.act = act; p.H = level_h[0]; p.Wd = level_w[0]; p.Cin = Cin; p.groups = 1;
  p.n_fastest = 1; p.dbg = g_gemm_dbg; p.splits = 1;
  // tile order: an XCD's wave of 32 workgroups = 16 pixel tiles x 2 weight panels (round 5, tools/order_ab.py: 1356-1360 vs
  // 1321-1345 TF/s for the N-fastest 8 x 4 order on the one-wave-per-SIMD kernel; half the weight-panel bytes per wave).
  // tools: debug mode 40 = the 8 x 4 order, 42 = 32 pixel tiles x 1 weight panel
  p.group_m = -2;
  if (g_gemm_dbg == 40 || g_gemm_dbg == 60) p.group_m = 0;
  if (g_gemm_dbg == 42) p.group_m = -1;
  // round 5: the one-wave-per-SIMD K 64 kernel (1383-1393 vs 1286-1292 TF/s, profiles/r05_w4k64_epilogue.txt); debug mode 60 = the
  // ring ping-pong kernel (tools: A/B arm), also the fallback for maps of 2 GiB and more
  if (g_gemm_dbg != 60 && (size_t)rows * Cin * 2 < 0x7fffffffu) return launch_w4k64<2>(p, (hipStream_t)stream);
  return launch_pp32<2, false, 256, 256, true, 1>(p, (hipStream_t)stream);
}

}  // extern "C"
