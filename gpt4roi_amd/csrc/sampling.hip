// sampling.hip -- device-side token sampling for generate(do_sample=True) (gfx950).
//
// The reference samples through HF `generate(do_sample=True, temperature=0.2, ...)` (gpt4roi/app.py:293-300); HF applies
// its logits warpers in the order temperature -> top-k -> top-p (top_k = 50 and top_p = 1.0 are the GenerationConfig
// defaults of the pinned transformers) and then draws from the remaining distribution.  This kernel is that step with the
// token id, position and step counter resident on the device (so the per-token decode step stays hipGraph-replayable,
// like g4r_greedy_advance_f32) and a counter-based generator: the uniform of step s is Philox4x32-10(counter = (s,0,0,0),
// key = seed) -- reproducible for a fixed seed whatever the launch geometry.  The draw is an inverse CDF over the kept
// tokens in ascending vocabulary order; oracle/sampler_oracle.py restates it (and is pinned to the Random123 known-answer
// vectors for Philox).
#include "g4r_common.h"

namespace {

__device__ __forceinline__ uint32_t order_key(float x) {          // monotone float -> uint map
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

constexpr int LIST_CAP = 1024;

// One workgroup of 1024 threads.  top_k in [1, LIST_CAP]: list path (kept tokens gathered into LDS, everything else by
// thread 0 on <= ~top_k entries).  top_k == 0: every token kept, chunked inverse CDF (top_p must be 1).
// The logits row is staged ONCE in LDS (`in_lds`: N * 4 B of dynamic LDS, 128 KB for the 32 006-token vocabulary) and the
// six passes over it (max, four radix-select passes, gather) read it from there; the first version walked the row in
// global memory with 256 threads, ~140 us per token.
constexpr int SNT = 1024;

struct SampleLds {                         // the static LDS of one draw (~15 KB)
  float red[SNT];
  unsigned hist[256];
  unsigned sel_prefix, sel_mask, sel_k, list_n;
  int list_idx[LIST_CAP];
  float list_e[LIST_CAP];
  double chunk_sum[256];
};

// One draw from the row `glogits[0, N)` with the uniform u: the body of the batch-1 and the batched sampler.  Every thread
// of the workgroup calls it; the token id is valid in thread 0 only.  `staged`: N floats of dynamic LDS when in_lds.
__device__ __forceinline__ int sample_row(const float* __restrict__ glogits, int N, int in_lds, float* staged,
                                          float inv_temp, int top_k, float top_p, float u, SampleLds& sh) {
  const int tid = threadIdx.x;
  float* red = sh.red;
  unsigned* hist = sh.hist;
  int* list_idx = sh.list_idx;
  float* list_e = sh.list_e;
  double* chunk_sum = sh.chunk_sum;
  const float* logits = glogits;
  if (in_lds) {
    for (int i = tid; i < N; i += SNT) staged[i] = glogits[i];
    __syncthreads();
    logits = staged;
  }
  // ---- max logit ----
  float m = -INFINITY;
  for (int i = tid; i < N; i += SNT) m = fmaxf(m, logits[i]);
  red[tid] = m;
  __syncthreads();
  for (int s = SNT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  int choice = -1;
  const int k_eff = top_k < N ? top_k : N;   // HF: top_k = min(top_k, vocabulary)
  uint32_t kth = 0;                          // order key of the k-th largest logit (0: every token kept)
  bool use_list = false;
  if (top_k >= 1 && (k_eff < N || N <= LIST_CAP)) {
    // ---- k-th largest logit by MSB radix select on the order-preserving key (ties with the k-th are all kept, as
    //      HF's TopKLogitsWarper does: scores < kth are removed) ----
    if (tid == 0) { sh.sel_prefix = 0; sh.sel_mask = 0; sh.sel_k = (unsigned)k_eff; }
    for (int pass = 3; pass >= 0; --pass) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned pre = sh.sel_prefix, msk = sh.sel_mask;
      const int shift = pass * 8;
      for (int i = tid; i < N; i += SNT) {
        const uint32_t k = order_key(logits[i]);
        if ((k & msk) == pre) atomicAdd(&hist[(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned cum = 0, k_rem = sh.sel_k;
        int b = 255;
        for (; b > 0; --b) {
          if (cum + hist[b] >= k_rem) break;
          cum += hist[b];
        }
        sh.sel_k = k_rem - cum;
        sh.sel_prefix = pre | ((unsigned)b << shift);
        sh.sel_mask = msk | (255u << shift);
      }
      __syncthreads();
    }
    kth = sh.sel_prefix;
    if (tid == 0) sh.list_n = 0;
    __syncthreads();
    for (int i = tid; i < N; i += SNT) {
      const float l = logits[i];
      if (order_key(l) >= kth) {
        const unsigned slot = atomicAdd(&sh.list_n, 1u);
        if (slot < LIST_CAP) {
          list_idx[slot] = i;
          list_e[slot] = expf((l - m) * inv_temp);
        }
      }
    }
    __syncthreads();
    // more than LIST_CAP tokens tie at the k-th logit (degenerate rows, e.g. constant logits): the kept set does not
    // fit the list -> chunked draw over the tokens with key >= kth below (top_p is not applied in that case)
    use_list = sh.list_n <= (unsigned)LIST_CAP;
    if (use_list) {
      // ascending vocabulary order by rank: entry a goes to slot #{b : idx[b] < idx[a]} (the indices are distinct); one
      // thread per entry instead of thread 0's insertion sort (~30 us at top_k = 50)
      const int n = (int)sh.list_n;
      int my_i = 0, rank = 0;
      float my_e = 0.f;
      if (tid < n) {
        my_i = list_idx[tid];
        my_e = list_e[tid];
        for (int b = 0; b < n; ++b) rank += list_idx[b] < my_i;
      }
      __syncthreads();
      if (tid < n) { list_idx[rank] = my_i; list_e[rank] = my_e; }
      __syncthreads();
    }
    if (use_list && tid == 0) {
      int n = (int)sh.list_n;
      double Z = 0.0;
      for (int a = 0; a < n; ++a) Z += (double)list_e[a];
      if (top_p < 1.0f) {
        // HF TopPLogitsWarper: a token stays iff the probability mass of the STRICTLY more probable tokens is < top_p
        // (ties ordered by vocabulary index); at least one token stays.
        for (int a = 0; a < n; ++a) {
          double above = 0.0;
          for (int b = 0; b < n; ++b)
            if (list_e[b] > list_e[a] || (list_e[b] == list_e[a] && list_idx[b] < list_idx[a])) above += (double)list_e[b];
          if (!(above < (double)top_p * Z)) list_idx[a] = -1 - list_idx[a];   // mark removed
        }
        double Z2 = 0.0;
        for (int a = 0; a < n; ++a)
          if (list_idx[a] >= 0) Z2 += (double)list_e[a];
        Z = Z2;
      }
      const double target = (double)u * Z;
      double acc = 0.0;
      int last = -1;
      for (int a = 0; a < n; ++a) {
        if (list_idx[a] < 0) continue;
        last = list_idx[a];
        acc += (double)list_e[a];
        if (acc > target) { choice = last; break; }
      }
      if (choice < 0) choice = last;
    }
  }
  if (!use_list) {
    // ---- chunked inverse CDF in ascending vocabulary order over the tokens with key >= kth (kth = 0: all) ----
    const int chunk = (N + 255) / 256;
    if (tid < 256) {
      const int c0 = tid * chunk, c1 = min(N, c0 + chunk);
      double s = 0.0;
      for (int i = c0; i < c1; ++i)
        if (order_key(logits[i]) >= kth) s += (double)expf((logits[i] - m) * inv_temp);
      chunk_sum[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
      double Z = 0.0;
      for (int c = 0; c < 256; ++c) Z += chunk_sum[c];
      const double target = (double)u * Z;
      double acc = 0.0;
      int c = 0;
      for (; c < 255; ++c) {
        if (acc + chunk_sum[c] > target) break;
        acc += chunk_sum[c];
      }
      const int b0 = c * chunk, b1 = min(N, b0 + chunk);
      choice = -1;
      for (int i = b0; i < b1; ++i) {
        if (order_key(logits[i]) < kth) continue;
        choice = i;                       // the last kept token seen: the fallback if rounding leaves acc <= target
        acc += (double)expf((logits[i] - m) * inv_temp);
        if (acc > target) break;
      }
      if (choice < 0)                     // rounding pushed the target past the last chunk: the last kept token
        for (int i = N - 1; i >= 0; --i)
          if (order_key(logits[i]) >= kth) { choice = i; break; }
    }
  }
  return choice < 0 ? 0 : choice;
}

// The uniform of step `st` for a 64-bit seed: 24 bits of Philox4x32-10(counter = (st,0,0,0), key = seed)[0] in [0, 1).
__device__ __forceinline__ float step_uniform(int st, unsigned long long sd) {
  uint32_t r4[4];
  philox4x32_10((uint32_t)st, 0u, 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), r4);
  return (float)(r4[0] >> 8) * (1.0f / 16777216.0f);
}

__global__ __launch_bounds__(SNT) void sample_advance_kernel(const float* __restrict__ glogits, int N, int in_lds, float inv_temp,
                                                             int top_k, float top_p,
                                                             const unsigned long long* __restrict__ seed,
                                                             long* __restrict__ tok, long* __restrict__ out_ids,
                                                             int* __restrict__ step, int* __restrict__ pos,
                                                             int max_steps, float* __restrict__ u_out) {
  extern __shared__ __attribute__((aligned(16))) float staged[];
  __shared__ SampleLds sh;
  const int st = *step;
  const float u = step_uniform(st, seed ? *seed : 0ull);
  const int choice = sample_row(glogits, N, in_lds, staged, inv_temp, top_k, top_p, u, sh);
  if (threadIdx.x == 0) {
    tok[0] = choice;
    if (st < max_steps) out_ids[st] = choice;
    if (u_out && st < max_steps) u_out[st] = u;
    *step = st + 1;
    *pos = *pos + 1;
  }
}

// Batched draw: workgroup b = row b with its own temperature / top-k / top-p / seed, all read from device memory (one
// captured graph serves any mix).  temperature[b] <= 0: greedy row, the argmax with the lowest index on ties -- the id
// g4r_argmax_rows_f32 returns.  Reads *step, never writes it: g4r_batch_advance moves the counters afterwards.
__global__ __launch_bounds__(SNT) void sample_rows_kernel(const float* __restrict__ glogits, long ld, int N, int in_lds,
                                                          const float* __restrict__ temperature,
                                                          const int* __restrict__ top_k, const float* __restrict__ top_p,
                                                          const unsigned long long* __restrict__ seed,
                                                          const int* __restrict__ step, long* __restrict__ next_ids,
                                                          float* __restrict__ u_out, int u_stride) {
  extern __shared__ __attribute__((aligned(16))) float staged[];
  __shared__ SampleLds sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = glogits + (size_t)b * ld;
  const int st = *step;
  const float u = step_uniform(st, seed[b]);
  const float t = temperature[b];
  int choice;
  if (t <= 0.f) {
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int i = tid; i < N; i += SNT) {
      const float v = row[i];
      if (v > best || (v == best && i < idx)) { best = v; idx = i; }
    }
    sh.red[tid] = best;
    sh.list_idx[tid] = idx;
    __syncthreads();
    for (int s = SNT / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const float v = sh.red[tid + s];
        const int i = sh.list_idx[tid + s];
        if (v > sh.red[tid] || (v == sh.red[tid] && i < sh.list_idx[tid])) { sh.red[tid] = v; sh.list_idx[tid] = i; }
      }
      __syncthreads();
    }
    choice = sh.list_idx[0];
  } else {
    const int k = min(max(top_k[b], 0), LIST_CAP);
    choice = sample_row(row, N, in_lds, staged, 1.0f / t, k, top_p[b], u, sh);
  }
  if (tid == 0) {
    next_ids[b] = choice;
    if (u_out && st < u_stride) u_out[(size_t)b * u_stride + st] = u;
  }
}

}  // namespace

extern "C" int g4r_sample_advance_f32(const float* logits, int N, float temperature, int top_k, float top_p,
                                      const unsigned long long* seed, long* tok, long* out_ids, int* step, int* pos,
                                      int max_steps, float* u_out, void* stream) {
  G4R_REQUIRE(logits && tok && out_ids && step && pos, "sample_advance: null pointer");
  G4R_REQUIRE(N > 0 && temperature > 0.f, "sample_advance: N > 0 and temperature > 0");
  G4R_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample_advance: top_p in (0, 1]");
  G4R_REQUIRE(top_k >= 0 && top_k <= LIST_CAP, "sample_advance: top_k in [0, 1024] (0 = disabled)");
  if (top_p < 1.f && !(top_k >= 1 && (top_k < N || N <= LIST_CAP)))
    return g4r_note_error(G4R_ERR_UNSUPPORTED, "sample_advance: top_p < 1 needs top_k in [1, 1024] (below the vocabulary size)");
  const int in_lds = (size_t)N * 4 <= 140 * 1024;       // + 15 KB of static LDS: within the 160 KB of a CU
  const size_t lds = in_lds ? (size_t)N * 4 : 0;
  static G4rPerDeviceOnce attr_set;
  if (attr_set.first()) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_advance_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024);
    if (e != hipSuccess) { attr_set.failed(); return g4r_note_hip_error(e, "sample_advance: hipFuncSetAttribute"); }
  }
  hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(SNT), lds, (hipStream_t)stream, logits, N, in_lds,
                     1.0f / temperature, top_k, top_p, seed, tok, out_ids, step, pos, max_steps, u_out);
  G4R_CHECK_LAUNCH("sample_advance");
  return G4R_OK;
}

extern "C" int g4r_sample_rows_f32(const float* logits, long row_stride, int B, int N, const float* temperature,
                                   const int* top_k, const float* top_p, const unsigned long long* seed, const int* step,
                                   long* next_ids, float* u_out, int u_stride, void* stream) {
  G4R_REQUIRE(logits && temperature && top_k && top_p && seed && step && next_ids, "sample_rows: null pointer");
  G4R_REQUIRE(B > 0 && N > 0 && row_stride >= N, "sample_rows: B > 0, N > 0, row_stride >= N");
  G4R_REQUIRE(!u_out || u_stride > 0, "sample_rows: u_stride > 0 with u_out");
  const int in_lds = (size_t)N * 4 <= 140 * 1024;
  const size_t lds = in_lds ? (size_t)N * 4 : 0;
  static G4rPerDeviceOnce attr_set;
  if (attr_set.first()) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_rows_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024);
    if (e != hipSuccess) { attr_set.failed(); return g4r_note_hip_error(e, "sample_rows: hipFuncSetAttribute"); }
  }
  hipLaunchKernelGGL(sample_rows_kernel, dim3(B), dim3(SNT), lds, (hipStream_t)stream, logits, row_stride, N, in_lds,
                     temperature, top_k, top_p, seed, step, next_ids, u_out, u_stride);
  G4R_CHECK_LAUNCH("sample_rows");
  return G4R_OK;
}
