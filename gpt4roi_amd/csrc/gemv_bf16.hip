// gemv_bf16.hip -- the single-row GEMV family (gemv_bf16_kernel): the decode step's projections, with the RMSNorm or the
// decode-attention merge in front of them fused in.  Entry points: gemm_bf16.hip (through gemv_dispatch).
#include "gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// GEMV for the single-token decode step (M = 1): pure weight streaming, HBM-bound (13.5 GB of bf16
// LLaMA-7B weights per token).  One wave owns 4 consecutive W rows; lanes split K in 16-byte
// pieces (one coalesced 1 KiB load per row per step, 4 rows in flight), fp32 accumulate, shuffle
// reduction.  Same epilogues as the GEMM (bias, residual, SwiGLU over interleaved row pairs, fp32 out).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void unpack8_h16(const uint4v& r, float* f) {
  f[0] = h16lo(r.x); f[1] = h16hi(r.x); f[2] = h16lo(r.y); f[3] = h16hi(r.y);
  f[4] = h16lo(r.z); f[5] = h16hi(r.z); f[6] = h16lo(r.w); f[7] = h16hi(r.w);
}

__device__ __forceinline__ float dot8_bf16(const uint4v& a, const uint4v& b, float acc) {
  acc += h16lo(a.x) * h16lo(b.x); acc += h16hi(a.x) * h16hi(b.x);
  acc += h16lo(a.y) * h16lo(b.y); acc += h16hi(a.y) * h16hi(b.y);
  acc += h16lo(a.z) * h16lo(b.z); acc += h16hi(a.z) * h16hi(b.z);
  acc += h16lo(a.w) * h16lo(b.w); acc += h16hi(a.w) * h16hi(b.w);
  return acc;
}

// x is staged ONCE per workgroup in LDS (the 4 waves of a workgroup would otherwise each re-read it from L2: K*2 B per
// wave against R*K*2 B of weights).  NORM fuses the RMSNorm that precedes the q|k|v, gate|up and lm_head projections
// (HF LlamaRMSNorm; same staging pattern, summation order and roundings as rmsnorm_bf16_kernel in norm.hip, so the
// normalised vector is bit-identical to the separate launch it replaces).  A wave owns R consecutive W rows and keeps
// R*U 16-byte loads in flight per lane (U K-steps of 1 KiB per row); shipped: R = 2, U = 8.
// XMODE 0: x as it is; 1: fused RMSNorm (gamma, eps); 2: x = the attention output assembled from the per-split partials
// the decode attention leaves behind (attention.hip, attn_decode_kernel with defer_merge): `gamma` then points at
// ws [H][S][D + 2] (un-normalised o, running max m, sum l per split), mS = S, mD = D.  Doing the merge in the consumer's
// staging loop replaces a cross-workgroup hand-off inside the attention launch (sc1 write-through, arrival counter, sc1
// read-back: ~6 us of serial memory round trips per layer) by a kernel boundary that is there anyway.
template <int R, int U, int XMODE, int NWV, int MAXV = 4>
__global__ __launch_bounds__(NWV * 64) void gemv_bf16_kernel(const h16_t* __restrict__ x, const float* __restrict__ gamma,
                                                        float eps, int mS, int mD, const h16_t* __restrict__ W,
                                                        void* __restrict__ C,
                                                        const float* __restrict__ bias,
                                                        const h16_t* __restrict__ residual, int N, int K, int ldw,
                                                        int act, int out_f32, int early_on) {
  extern __shared__ __attribute__((aligned(16))) char gemv_smem[];
  uint4v* xs = reinterpret_cast<uint4v*>(gemv_smem);
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nvec = K >> 3;
  const int n0 = (blockIdx.x * NWV + wave) * R;
  const h16_t* wrow[R];
#pragma unroll
  for (int r = 0; r < R; ++r) wrow[r] = W + (size_t)(n0 + r < N ? n0 + r : N - 1) * ldw;
  uint4v wv[U][R];
  auto load_w = [&](int vb) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = vb + 64 * u < nvec ? vb + 64 * u : nvec - 1;
#pragma unroll
      for (int r = 0; r < R; ++r)
        wv[u][r] = __builtin_nontemporal_load(reinterpret_cast<const uint4v*>(wrow[r] + (size_t)idx * 8));
    }
  };
  // Round 6: every wave issues its first block of weight loads right AFTER the loads of its share of the staging and BEFORE it
  // waits for them: vector memory returns in order, so the x loads (older) are not delayed and the weight stream runs from the
  // first cycles of the workgroup instead of after the 2-3 memory round trips + 2 barriers of the staging.  Same loads, same
  // arithmetic, same bits.  (The other order -- weights first, then x -- queues x behind R*U HBM loads: 5-8 % slower, round 2.)
  const bool early = early_on && n0 < N;   // (early_on = 0: debug mode 62, the A/B of tools/decode_bench.py)
  bool pre = false;                        // the first block of W is already in flight when the main loop starts
  if (XMODE == 1) {
    // the first 4 waves stage and normalise x exactly as rmsnorm_bf16_kernel's 256 threads do (same element -> thread
    // map and summation order: bit-identical rstd); further waves of a wide workgroup only wait at the barriers
    // MAXV vectors of 8 per staging thread: K <= 2048 * MAXV (the launcher picks 2 for K <= 4096, else 4; K <= 8192 checked there).
    // x stays PACKED in registers and is unpacked twice: with the first weight block (R*U*4 registers) in flight next to x and
    // gamma the kernel must stay under 80 registers, or a CU no longer holds three workgroups (the wide projections launch 3-8 per CU)
    uint4v xr[MAXV];
    // gamma: the waves that do not stage x (4..NWV-1) fetch it next to the x loads of the stagers and park it in LDS behind x, so
    // its round trip no longer follows the two barriers of the reduction and costs the stagers no registers
    constexpr bool GLDS = NWV > 4;
    constexpr int GW = GLDS ? (NWV - 4) * 64 : 1;
    float* gs = reinterpret_cast<float*>(gemv_smem + (size_t)K * 2);
    float4v gq[GLDS ? 2 * MAXV : 1];
    float s2 = 0.f;
    const bool stager = tid < 256;
    if (stager) {
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int v = tid + i * 256;
        if (v < nvec) xr[i] = *reinterpret_cast<const uint4v*>(x + v * 8);
      }
    } else if (GLDS) {
#pragma unroll
      for (int i = 0; i < 2 * MAXV; ++i) {
        const int v4 = tid - 256 + i * GW;
        if (v4 < (K >> 2)) gq[i] = *reinterpret_cast<const float4v*>(gamma + v4 * 4);
      }
    }
    if (early) { load_w(lane); pre = true; }
    if (stager) {
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int v = tid + i * 256;
        if (v < nvec) {
          float fx[8];
          unpack8_h16(xr[i], fx);
#pragma unroll
          for (int k = 0; k < 8; ++k) s2 += fx[k] * fx[k];
        }
      }
    } else if (GLDS) {
#pragma unroll
      for (int i = 0; i < 2 * MAXV; ++i) {
        const int v4 = tid - 256 + i * GW;
        if (v4 < (K >> 2)) *reinterpret_cast<float4v*>(gs + v4 * 4) = gq[i];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
    __syncthreads();
    if (lane == 0 && stager) red[wave] = s2;
    __syncthreads();
    const float rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = tid + i * 256;
      if (stager && v < nvec) {
        const float* gp = GLDS ? gs + v * 8 : gamma + v * 8;
        const float4v g0 = *reinterpret_cast<const float4v*>(gp);
        const float4v g1 = *reinterpret_cast<const float4v*>(gp + 4);
        const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        float o[8], fx[8];
        unpack8_h16(xr[i], fx);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = h16_to_f32(f32_to_h16(fx[k] * rstd)) * g[k];
        uint4v w;
        w.x = pack_h16x2(o[0], o[1]); w.y = pack_h16x2(o[2], o[3]);
        w.z = pack_h16x2(o[4], o[5]); w.w = pack_h16x2(o[6], o[7]);
        xs[v] = w;
      }
    }
  } else if (XMODE == 2) {
    const int SLD = mD + 2;
    constexpr int MS = 8;            // splits whose partials one thread holds in registers (the decode step uses 8)
    float pm[MS], pl[MS];
    float4v po0[MS], po1[MS];
    auto part_of = [&](int v, int& d0) {
      const int h = (v * 8) / mD;
      d0 = (v * 8) - h * mD;
      return gamma + (size_t)h * mS * SLD;
    };
    auto mload = [&](int v) {        // every load of the merge of one 8-element vector, issued together
      int d0;
      const float* part = part_of(v, d0);
#pragma unroll
      for (int i = 0; i < MS; ++i) {
        if (i < mS) {
          pm[i] = part[i * SLD + mD];
          pl[i] = part[i * SLD + mD + 1];
          po0[i] = *reinterpret_cast<const float4v*>(part + i * SLD + d0);
          po1[i] = *reinterpret_cast<const float4v*>(part + i * SLD + d0 + 4);
        }
      }
    };
    auto mfinish = [&](int v) {      // the arithmetic of the loop form below, term for term
      float mm = -INFINITY;
#pragma unroll
      for (int i = 0; i < MS; ++i)
        if (i < mS) mm = fmaxf(mm, pm[i]);
      float Lt = 0.f, a2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < MS; ++i) {
        if (i < mS) {
          const float w = pm[i] == -INFINITY ? 0.f : exp2f(pm[i] - mm);
          Lt += w * pl[i];
          a2[0] += w * po0[i].x; a2[1] += w * po0[i].y; a2[2] += w * po0[i].z; a2[3] += w * po0[i].w;
          a2[4] += w * po1[i].x; a2[5] += w * po1[i].y; a2[6] += w * po1[i].z; a2[7] += w * po1[i].w;
        }
      }
      uint4v w8;
      w8.x = pack_h16x2(a2[0] / Lt, a2[1] / Lt); w8.y = pack_h16x2(a2[2] / Lt, a2[3] / Lt);
      w8.z = pack_h16x2(a2[4] / Lt, a2[5] / Lt); w8.w = pack_h16x2(a2[6] / Lt, a2[7] / Lt);
      xs[v] = w8;
    };
    if (mS <= MS) {
      int v = tid;
      if (v < nvec) mload(v);
      if (early) { load_w(lane); pre = true; }
      if (v < nvec) mfinish(v);
      for (v += NWV * 64; v < nvec; v += NWV * 64) {
        mload(v);
        mfinish(v);
      }
    } else {
      for (int v = tid; v < nvec; v += NWV * 64) {
        int d0;
        const float* part = part_of(v, d0);
        float mm = -INFINITY;
        for (int i = 0; i < mS; ++i) mm = fmaxf(mm, part[i * SLD + mD]);
        float Lt = 0.f, a2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < mS; ++i) {
          const float mi = part[i * SLD + mD];
          const float w = mi == -INFINITY ? 0.f : exp2f(mi - mm);
          Lt += w * part[i * SLD + mD + 1];
          const float4v o0 = *reinterpret_cast<const float4v*>(part + i * SLD + d0);
          const float4v o1 = *reinterpret_cast<const float4v*>(part + i * SLD + d0 + 4);
          a2[0] += w * o0.x; a2[1] += w * o0.y; a2[2] += w * o0.z; a2[3] += w * o0.w;
          a2[4] += w * o1.x; a2[5] += w * o1.y; a2[6] += w * o1.z; a2[7] += w * o1.w;
        }
        uint4v w8;
        w8.x = pack_h16x2(a2[0] / Lt, a2[1] / Lt); w8.y = pack_h16x2(a2[2] / Lt, a2[3] / Lt);
        w8.z = pack_h16x2(a2[4] / Lt, a2[5] / Lt); w8.w = pack_h16x2(a2[6] / Lt, a2[7] / Lt);
        xs[v] = w8;
      }
    }
  } else {
    constexpr int XPRE = 3;          // x vectors per thread held in registers across the early weight loads (K <= 12288 at 8 waves)
    uint4v xr[XPRE];
#pragma unroll
    for (int i = 0; i < XPRE; ++i) {
      const int v = tid + i * NWV * 64;
      if (v < nvec) xr[i] = *reinterpret_cast<const uint4v*>(x + v * 8);
    }
    if (early) { load_w(lane); pre = true; }
#pragma unroll
    for (int i = 0; i < XPRE; ++i) {
      const int v = tid + i * NWV * 64;
      if (v < nvec) xs[v] = xr[i];
    }
    for (int v = tid + XPRE * NWV * 64; v < nvec; v += NWV * 64) xs[v] = *reinterpret_cast<const uint4v*>(x + v * 8);
  }
  __syncthreads();
  if (n0 >= N) return;
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  for (int vb = lane; vb < nvec; vb += 64 * U) {
    if (!(pre && vb == lane)) load_w(vb);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (vb + 64 * u < nvec) {
        const uint4v xv = xs[vb + 64 * u];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = dot8_bf16(xv, wv[u][r], acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o);
  if (lane != 0) return;
  if (act == 4) {  // rows are (gate, up) pairs
#pragma unroll
    for (int r = 0; r < R; r += 2) {
      if (n0 + r + 1 < N) {
        const float g = acc[r], u = acc[r + 1];
        const float sg = h16lo(pack_h16x2(g / (1.f + __expf(-g)), 0.f));
        reinterpret_cast<h16_t*>(C)[(n0 + r) >> 1] = f32_to_h16(sg * u);
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int n = n0 + r;
    if (n >= N) break;
    float vv = acc[r];
    if (bias) vv += bias[n];
    vv = apply_act(vv, act);
    if (residual) vv += h16_to_f32(residual[n]);
    if (out_f32)
      reinterpret_cast<float*>(C)[n] = vv;
    else
      reinterpret_cast<h16_t*>(C)[n] = f32_to_h16(vv);
  }
}

template <int R, int U, int NWV>
static void launch_gemv(int xmode, const h16_t* x, const float* gamma, float eps, int mS, int mD, const h16_t* W, void* C,
                        const float* bias, const h16_t* residual, int N, int K, int ldw, int act, int out_f32,
                        hipStream_t stream) {
  const int waves = g4r_ceil_div(N, R);
  const dim3 grid(g4r_ceil_div(waves, NWV)), block(NWV * 64);
  const size_t lds = (size_t)K * 2 + (xmode == 1 && NWV > 4 ? (size_t)K * 4 : 0);   // x, and gamma behind it (fused norm, wide workgroups)
  if (xmode == 1 && K <= 4096)
    hipLaunchKernelGGL((gemv_bf16_kernel<R, U, 1, NWV, 2>), grid, block, lds, stream, x, gamma, eps, mS, mD, W, C, bias,
                       residual, N, K, ldw, act, out_f32, g_gemm_dbg == 62 ? 0 : 1);
  else if (xmode == 1)
    hipLaunchKernelGGL((gemv_bf16_kernel<R, U, 1, NWV>), grid, block, lds, stream, x, gamma, eps, mS, mD, W, C, bias,
                       residual, N, K, ldw, act, out_f32, g_gemm_dbg == 62 ? 0 : 1);
  else if (xmode == 2)
    hipLaunchKernelGGL((gemv_bf16_kernel<R, U, 2, NWV>), grid, block, lds, stream, x, gamma, eps, mS, mD, W, C, bias,
                       residual, N, K, ldw, act, out_f32, g_gemm_dbg == 62 ? 0 : 1);
  else
    hipLaunchKernelGGL((gemv_bf16_kernel<R, U, 0, NWV>), grid, block, lds, stream, x, gamma, eps, mS, mD, W, C, bias,
                       residual, N, K, ldw, act, out_f32, g_gemm_dbg == 62 ? 0 : 1);
}

}  // namespace

// (R rows per wave, U K-steps in flight, waves per workgroup); variant >= 0: A/B probe (tools/gemm_bench.cpp v: cases)
void G4R_GEMM_NS::gemv_dispatch(int variant, int xmode, const h16_t* x, const float* gamma, float eps, int mS, int mD,
                                const h16_t* W, void* C, const float* bias, const h16_t* residual, int N, int K, int ldw,
                                int act, int out_f32, hipStream_t st) {
  if (variant < 0) variant = 2;   // R = 2, U = 4, 8 waves: best or within noise of the best on all five LLaMA-7B projections (profiles/r02_gemv_variants.txt)
#define G4R_GEMV_CASE(v, R_, U_, NW_) \
  case v: launch_gemv<R_, U_, NW_>(xmode, x, gamma, eps, mS, mD, W, C, bias, residual, N, K, ldw, act, out_f32, st); break;
  switch (variant) {
    G4R_GEMV_CASE(0, 4, 2, 4)
    G4R_GEMV_CASE(1, 2, 4, 4)
    G4R_GEMV_CASE(2, 2, 4, 8)
    G4R_GEMV_CASE(3, 2, 4, 16)
    G4R_GEMV_CASE(4, 2, 8, 4)
    G4R_GEMV_CASE(5, 2, 8, 8)
    G4R_GEMV_CASE(6, 4, 2, 8)
    default: launch_gemv<4, 4, 8>(xmode, x, gamma, eps, mS, mD, W, C, bias, residual, N, K, ldw, act, out_f32, st); break;
  }
#undef G4R_GEMV_CASE
}
