// Fused multi-tensor AdamW and the VQ codebook nearest-neighbour lookup (gfx950).
//
// AdamW: vae_trainer.py:455-475 (optimizer_G two param groups, optimizer_D), stepped at
// vae_trainer.py:659,702-704 — torch.optim.AdamW semantics, one launch for all tensors
// (28 B/param of HBM traffic: read p,g,m,v, write p,m,v; 36 B/param for a tensor that keeps an EMA shadow: + read and write of it).
// VQ: not in the reference; the algorithm is pinned by oracle/vq_oracle.c.
#include "vq_common.h"

// One chunk [beg, end) of one table entry.  EMA = false is the plain update; EMA = true additionally moves the tensor's shadow
// (VqAdamTensor::ema, include/vqhip.h) towards the value just stored to p:  ema += (p_new - ema) * (1 - d), torch's lerp_ form like the
// m update — 8 B/param more on a value the lane already holds, against 12 B/param and a second launch for a separate pass.
// EVEC (EMA only): the shadow is 16-byte aligned and goes 16 bytes per lane; else 4 bytes at a time.  Three instantiations of one
// body, chosen by block-uniform branches in the kernel: the `if constexpr` arms vanish from the plain one.  (EVEC is a template
// parameter and not a run-time flag: with a flag the compiler merged the two store arms into one — a 12-byte and a 4-byte store per
// quad also for an aligned shadow.)
template <bool EMA, bool EVEC, class Update>
__device__ __forceinline__ void adamw_chunk(const VqAdamTensor& t, int64_t beg, int64_t end, float ema_w, const Update& update) {
  auto shadow = [&](float& e, float p) { e = e + (p - e) * ema_w; };
  // 16 bytes per lane and array, two quads per trip (8 loads in flight per lane): scalar 4-byte accesses ran this pass at 3.5-3.8 TB/s
  // (r2 profiles).  Chunks start at multiples of 4 elements of 16-byte aligned buffers (vq_adamw_multi checks); the tail is scalar.
  const bool aligned = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0) && (beg & 3) == 0;
  // The shadow's 16-byte accesses need the shadow 16-byte aligned as well; one that is not goes by 4-byte accesses INSIDE the same
  // loops: which loop p / m / v run through, and with it their bits (the compiler contracts each loop's arithmetic on its own), must
  // not depend on where the shadow lies.
  float* const eb = EMA ? t.ema + beg : nullptr;
  auto load_e = [&](int64_t q) {
    vq_f4 e;
    if constexpr (EVEC) {
      e = ((const vq_f4*)eb)[q];
    } else {
      e.x = eb[4 * q]; e.y = eb[4 * q + 1]; e.z = eb[4 * q + 2]; e.w = eb[4 * q + 3];
    }
    return e;
  };
  auto store_e = [&](int64_t q, const vq_f4& e) {
    if constexpr (EVEC) {
      ((vq_f4*)eb)[q] = e;
    } else {
      eb[4 * q] = e.x; eb[4 * q + 1] = e.y; eb[4 * q + 2] = e.z; eb[4 * q + 3] = e.w;
    }
  };
  int64_t i = beg;
  if (aligned) {
    const int64_t nq = (end - beg) >> 2;
    vq_f4* __restrict__ p4 = (vq_f4*)(t.p + beg);
    const vq_f4* __restrict__ g4 = (const vq_f4*)(t.g + beg);
    vq_f4* __restrict__ m4 = (vq_f4*)(t.m + beg);
    vq_f4* __restrict__ v4 = (vq_f4*)(t.v + beg);
    int64_t q = threadIdx.x;
    for (; q + 256 < nq; q += 512) {
      vq_f4 p0 = p4[q], g0 = g4[q], m0 = m4[q], v0 = v4[q], p1 = p4[q + 256], g1 = g4[q + 256], m1 = m4[q + 256], v1 = v4[q + 256];
      update(g0.x, p0.x, m0.x, v0.x); update(g0.y, p0.y, m0.y, v0.y); update(g0.z, p0.z, m0.z, v0.z); update(g0.w, p0.w, m0.w, v0.w);
      update(g1.x, p1.x, m1.x, v1.x); update(g1.y, p1.y, m1.y, v1.y); update(g1.z, p1.z, m1.z, v1.z); update(g1.w, p1.w, m1.w, v1.w);
      p4[q] = p0; m4[q] = m0; v4[q] = v0; p4[q + 256] = p1; m4[q + 256] = m1; v4[q + 256] = v1;
      if constexpr (EMA) {
        vq_f4 e0 = load_e(q), e1 = load_e(q + 256);
        shadow(e0.x, p0.x); shadow(e0.y, p0.y); shadow(e0.z, p0.z); shadow(e0.w, p0.w);
        shadow(e1.x, p1.x); shadow(e1.y, p1.y); shadow(e1.z, p1.z); shadow(e1.w, p1.w);
        store_e(q, e0); store_e(q + 256, e1);
      }
    }
    for (; q < nq; q += 256) {
      vq_f4 p0 = p4[q], g0 = g4[q], m0 = m4[q], v0 = v4[q];
      update(g0.x, p0.x, m0.x, v0.x); update(g0.y, p0.y, m0.y, v0.y); update(g0.z, p0.z, m0.z, v0.z); update(g0.w, p0.w, m0.w, v0.w);
      p4[q] = p0; m4[q] = m0; v4[q] = v0;
      if constexpr (EMA) {
        vq_f4 e0 = load_e(q);
        shadow(e0.x, p0.x); shadow(e0.y, p0.y); shadow(e0.z, p0.z); shadow(e0.w, p0.w);
        store_e(q, e0);
      }
    }
    i = beg + (nq << 2);
  }
  for (i += threadIdx.x; i < end; i += 256) {
    float p = t.p[i], m = t.m[i], v = t.v[i];
    update(t.g[i], p, m, v);
    t.p[i] = p; t.m[i] = m; t.v[i] = v;
    if constexpr (EMA) {
      float e = t.ema[i];
      shadow(e, p);
      t.ema[i] = e;
    }
  }
}

__global__ __launch_bounds__(256) void adamw_multi_kernel(const VqAdamTensor* __restrict__ table,
                                                           const int64_t* __restrict__ chunk_offsets, int n_tensors,
                                                           int chunk, float lr, float wd, float beta1, float beta2,
                                                           float eps, float bc1, float bc2_sqrt, float grad_scale,
                                                           const int* __restrict__ skip_flags, int n_flags, int skip_stride) {
  // a step whose gradients were clipped by a saturating VQ_F16 store (range events, include/vqhip.h) changes nothing — the shadow
  // included: block-uniform
  for (int f = 0; f < n_flags; ++f)
    if (skip_flags[(int64_t)f * skip_stride] != 0) return;
  const int64_t cid = blockIdx.x;
  // binary search: largest t with chunk_offsets[t] <= cid
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_offsets[mid] <= cid) lo = mid; else hi = mid - 1;
  }
  const VqAdamTensor t = table[lo];
  const int64_t beg = (cid - chunk_offsets[lo]) * chunk;
  int64_t end = beg + chunk;
  if (end > t.n) end = t.n;
  const float decay = 1.f - lr * wd, step = lr / bc1;
  // (One lambda for every loop of every instantiation below.  That p / m / v do not depend on whether a tensor keeps a shadow, or on
  // where it lies, rests on the compiler contracting this arithmetic the same way in each copy of a loop: nothing in the language
  // promises that — the scalar tail, for one, rounds p differently from the vector loops on gfx950 — and only the bitwise comparison
  // with the no-shadow launch in tests/test_weight_ema.py, run on the GPU, guards it.)
  auto update = [&](float g, float& p, float& m, float& v) {
    g *= grad_scale;
    p *= decay;
    m = m + (g - m) * (1.f - beta1);                              // lerp_, as torch does
    v = v * beta2 + (1.f - beta2) * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p -= step * (m / denom);
  };
  if (!t.ema) adamw_chunk<false, false>(t, beg, end, 0.f, update);
  else if (((uintptr_t)t.ema & 15) == 0) adamw_chunk<true, true>(t, beg, end, 1.f - *t.ema_decay, update);   // (the decay: a device scalar,
  else adamw_chunk<true, false>(t, beg, end, 1.f - *t.ema_decay, update);                                   //  read here, nowhere on the host)
}

extern "C" int vq_adamw_multi(const VqAdamTensor* table, const int64_t* chunk_offsets, int n_tensors, int64_t total_chunks,
                              int chunk, float lr, float wd, float beta1, float beta2, float eps, float bc1, float bc2,
                              float grad_scale, const int32_t* skip_flags, int n_flags, int skip_stride, void* stream) {
  VQ_REQUIRE(table && chunk_offsets && n_tensors > 0 && chunk > 0, VQ_ERR_INVALID, "vq_adamw_multi: bad arguments");
  VQ_REQUIRE(n_flags >= 0 && n_flags <= 64 && (n_flags == 0 || (skip_flags && skip_stride > 0)), VQ_ERR_INVALID,
             "vq_adamw_multi: bad skip flags (n_flags=%d stride=%d)", n_flags, skip_stride);
  VQ_REQUIRE(total_chunks > 0 && total_chunks < (1ll << 31), VQ_ERR_INVALID, "vq_adamw_multi: bad chunk count");
  hipLaunchKernelGGL(adamw_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_offsets,
                     n_tensors, chunk, lr, wd, beta1, beta2, eps, bc1, sqrtf(bc2), grad_scale, (const int*)skip_flags,
                     skip_flags ? n_flags : 0, skip_stride);
  VQ_CHECK_LAUNCH("vq_adamw_multi");
  return VQ_OK;
}

// ------------------------------------------------------------------------------------------ VQ
// One thread per token (z row in registers), codebook streamed through LDS in tiles and read
// by broadcast; code range split over blockIdx.y; fixed-order fmaf chains (see oracle/vq_oracle.c):
//   zz = fma-chain_k z_k*z_k ; ee likewise ; dot = fma-chain_k z_k*e_k   (k ascending, start 0)
//   d  = (zz - 2*dot) + ee ;   strict '<' while scanning j ascending => lowest index wins ties.
static constexpr int VQ_TILE = 128;
template <int D>
__global__ __launch_bounds__(256) void vq_nearest_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                          int64_t n_tokens, int n_codes, int codes_per_split,
                                                          float* __restrict__ pmin, int* __restrict__ pidx) {
  __shared__ __attribute__((aligned(16))) float tile[VQ_TILE * D];
  __shared__ float tee[VQ_TILE];
  const int64_t tok = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = tok < n_tokens;
  float zr[D];
  float zz = 0.f;
#pragma unroll
  for (int k = 0; k < D; ++k) { zr[k] = live ? z[tok * D + k] : 0.f; zz = fmaf(zr[k], zr[k], zz); }
  const int jbeg = blockIdx.y * codes_per_split;
  int jend = jbeg + codes_per_split;
  if (jend > n_codes) jend = n_codes;
  float best = __uint_as_float(0x7f800000u);  // +inf
  int besti = jbeg;
  for (int j0 = jbeg; j0 < jend; j0 += VQ_TILE) {
    const int nt = (jend - j0) < VQ_TILE ? (jend - j0) : VQ_TILE;
    __syncthreads();
    for (int i = threadIdx.x; i < nt * D; i += 256) tile[i] = cb[(int64_t)j0 * D + i];
    __syncthreads();
    if (threadIdx.x < nt) {
      float ee = 0.f;
      for (int k = 0; k < D; ++k) ee = fmaf(tile[threadIdx.x * D + k], tile[threadIdx.x * D + k], ee);
      tee[threadIdx.x] = ee;
    }
    __syncthreads();
    for (int jj = 0; jj < nt; ++jj) {
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) dot = fmaf(zr[k], tile[jj * D + k], dot);
      const float d = (zz - 2.f * dot) + tee[jj];
      if (d < best) { best = d; besti = j0 + jj; }
    }
  }
  if (live) {
    pmin[(int64_t)blockIdx.y * n_tokens + tok] = best;
    pidx[(int64_t)blockIdx.y * n_tokens + tok] = besti;
  }
}

// The same search on the fp32 MFMA (v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate, the fp32 vector rate with none of the VALU's
// broadcast-read traffic).  It is EXACT f32 — per output element an fmaf chain over k onto the accumulator — so chaining D / 2
// instructions over k = (0,1), (2,3), ... reproduces `dot = fmaf(z_k, e_k, dot)`, k ascending, bit for bit (pinned to silicon by
// tests/test_hw_layout.py probe 5; the indices by tests/test_vq.py against oracle/vq_oracle.c at 8192 x 16384 x 32).
// One wave = 32 tokens (A operand: lane l holds token l & 31, components k = 2 s + (l >> 5): D / 2 registers, resident); the codebook
// goes through LDS in tiles of 128 codes, de-interleaved on the way in ([code][parity][D / 2]) so that a lane's D / 2 B-operand values are
// contiguous; per 32-code block D / 2 MFMAs leave dot(token, code) for 16 tokens x 1 code per lane; d = (zz - 2 dot) + ee and the
// strict '<' scan run on the VALU under the next block's MFMAs (two waves per SIMD); a (d, index) butterfly over the 32 lanes that
// hold one token's codes — smaller d, lower index on ties — ends the split.  zz / ee are the oracle's fmaf chains, on the VALU.
// |e_j|^2 of every code, the oracle's fmaf chain (k ascending): once per lookup, so the search blocks do not each redo it
template <int D>
__global__ __launch_bounds__(256) void vq_code_norms_kernel(const float* __restrict__ cb, int n_codes, float* __restrict__ ee) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_codes) return;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < D; ++k) { const float v = cb[(int64_t)j * D + k]; acc = fmaf(v, v, acc); }
  ee[j] = acc;
}

template <int D>
__global__ __launch_bounds__(256) void vq_nearest_mfma_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                               const float* __restrict__ ee_all, int64_t n_tokens, int n_codes,
                                                               int codes_per_split, float* __restrict__ pmin, int* __restrict__ pidx) {
  constexpr int KS = D / 2, CT = D <= 32 ? 128 : 64;  // codes per tile: two buffers stay within 37 KiB of LDS
  constexpr int RS = D + 4;                           // row stride in LDS: + 4 floats, so that the lanes' 16-byte reads spread over the banks
  constexpr int NF4 = CT * D / 4 / 256;               // float4 pieces of a tile per thread
  static_assert(D % 8 == 0 && D >= 8 && D <= 64 && NF4 >= 1, "code dimension");
  __shared__ __attribute__((aligned(16))) float tile[2][CT * RS];   // [code][parity][KS] (+ pad), two buffers
  __shared__ float tee[2][CT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int64_t tok0 = (int64_t)blockIdx.x * 128 + wave * 32;
  const int64_t tok = tok0 + fr;
  const bool live = tok < n_tokens;
  // A operand + the token's |z|^2 (full chain, k ascending: both halves of the wave compute it)
  float az[KS];
  float zz = 0.f;
  {
    const float* zr = z + (live ? tok : 0) * D;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const float v = live ? zr[k] : 0.f;
      zz = fmaf(v, v, zz);
      if ((k & 1) == fh) az[k >> 1] = v;
    }
  }
  // accumulator element e of a lane = token row (e & 3) + 8 (e >> 2) + 4 fh of the wave's 32
  float zzr[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) zzr[e] = __shfl(zz, (e & 3) + 8 * (e >> 2) + 4 * fh);
  const float inf = __uint_as_float(0x7f800000u);
  float best[16];
  int besti[16];                                      // first code of the 32-code block that holds the best one (+ fr = the code)
#pragma unroll
  for (int e = 0; e < 16; ++e) { best[e] = inf; besti[e] = 0; }
  const int jbeg = blockIdx.y * codes_per_split;
  int jend = jbeg + codes_per_split;
  if (jend > n_codes) jend = n_codes;
  // tile staging through registers: the next tile's global loads are in flight under this tile's MFMAs
  float4 pf[NF4];
  float pe = 0.f;
  auto fetch = [&](int j0) {
    const int nt = (jend - j0) < CT ? (jend - j0) : CT;
#pragma unroll
    for (int u = 0; u < NF4; ++u) {
      const int i = tid + u * 256, code = i / (D / 4), q = i - code * (D / 4);
      pf[u] = code < nt ? *(const float4*)(cb + (int64_t)(j0 + code) * D + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    pe = (tid < nt) ? ee_all[j0 + tid] : inf;         // rows past the split's end: |e|^2 = +inf, never the minimum
  };
  auto stash = [&](int buf) {                       // de-interleave: k = 4q, 4q + 2 -> parity 0; 4q + 1, 4q + 3 -> parity 1
#pragma unroll
    for (int u = 0; u < NF4; ++u) {
      const int i = tid + u * 256, code = i / (D / 4), q = i - code * (D / 4);
      float* dst = &tile[buf][code * RS];
      *(float2*)(dst + 2 * q) = make_float2(pf[u].x, pf[u].z);
      *(float2*)(dst + KS + 2 * q) = make_float2(pf[u].y, pf[u].w);
    }
    if (tid < CT) tee[buf][tid] = pe;
  };
  auto load_b = [&](float (&bz)[KS], int buf, int cb0) {
    const float* bsrc = &tile[buf][(cb0 + fr) * RS + fh * KS];
#pragma unroll
    for (int q = 0; q < KS / 4; ++q) {
      const float4 v = *(const float4*)(bsrc + q * 4);
      bz[q * 4] = v.x; bz[q * 4 + 1] = v.y; bz[q * 4 + 2] = v.z; bz[q * 4 + 3] = v.w;
    }
  };
  if (jbeg < jend) { fetch(jbeg); stash(0); }
  __syncthreads();
  int buf = 0;
  for (int j0 = jbeg; j0 < jend; j0 += CT, buf ^= 1) {
    const bool more = j0 + CT < jend;
    if (more) fetch(j0 + CT);
    float bz[2][KS];
    load_b(bz[0], buf, 0);
#pragma unroll
    for (int c = 0; c < CT / 32; ++c) {                // (all CT rows: rows past the split's end are zeros with |e|^2 = +inf)
      if (c + 1 < CT / 32) load_b(bz[(c + 1) & 1], buf, (c + 1) * 32);
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int sidx = 0; sidx < KS; ++sidx) acc = mfma_32x32x2_f32(az[sidx], bz[c & 1][sidx], acc);
      const float ee = tee[buf][c * 32 + fr];
      const int blk = j0 + c * 32;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float d = (zzr[e] - 2.f * acc[e]) + ee;
        const bool lt = d < best[e];
        best[e] = lt ? d : best[e];
        besti[e] = lt ? blk : besti[e];
      }
    }
    if (more) stash(buf ^ 1);                        // (buffer buf ^ 1 was last read one tile ago: behind the barrier below)
    __syncthreads();
  }
  // One token's candidates sit in the 32 lanes of a half wave (one code residue each): smaller d wins, the lower index on ties.
  // Halving exchange: at distance 16, 8, 4, 2 a lane keeps the half of its elements its lane bit selects and merges the partner's
  // copy of them — 8 + 4 + 2 + 1 merges instead of 16 per distance — then one merge at distance 1.
  float b[16];
  int bi[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) { b[e] = best[e]; bi[e] = besti[e] + fr; }
#pragma unroll
  for (int lvl = 0; lvl < 4; ++lvl) {
    const int m = 16 >> lvl, n = 8 >> lvl;          // lane distance, elements kept
    const bool up = (fr & m) != 0;
#pragma unroll
    for (int e = 0; e < n; ++e) {
      const float keep = up ? b[e + n] : b[e], send = up ? b[e] : b[e + n];
      const int keepi = up ? bi[e + n] : bi[e], sendi = up ? bi[e] : bi[e + n];
      const float ob = __shfl_xor(send, m);
      const int oi = __shfl_xor(sendi, m);
      const bool take = ob < keep || (ob == keep && oi < keepi);
      b[e] = take ? ob : keep;
      bi[e] = take ? oi : keepi;
    }
  }
  {
    const float ob = __shfl_xor(b[0], 1);
    const int oi = __shfl_xor(bi[0], 1);
    if (ob < b[0] || (ob == b[0] && oi < bi[0])) { b[0] = ob; bi[0] = oi; }
  }
  // the element a lane ends with: bit 3 <- lane bit 4, bit 2 <- bit 3, bit 1 <- bit 2, bit 0 <- bit 1
  const int e_mine = fr >> 1;
  const int64_t t = tok0 + (e_mine & 3) + 8 * (e_mine >> 2) + 4 * fh;
  if ((fr & 1) == 0 && t < n_tokens) {
    pmin[(int64_t)blockIdx.y * n_tokens + t] = b[0];
    pidx[(int64_t)blockIdx.y * n_tokens + t] = bi[0];
  }
}

// The end of a split as in vq_nearest_mfma_kernel (which keeps its own copy, so that its instruction stream stays the measured one):
// the halving exchange over the 32 lanes that hold one token's codes, smaller d first, the lower index on ties.
__device__ __forceinline__ void vq_mfma_split_store(const float (&best)[16], const int (&besti)[16], int fr, int fh, int64_t tok0,
                                                    int64_t n_tokens, float* __restrict__ pmin, int* __restrict__ pidx) {
  float b[16];
  int bi[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) { b[e] = best[e]; bi[e] = besti[e] + fr; }
#pragma unroll
  for (int lvl = 0; lvl < 4; ++lvl) {
    const int m = 16 >> lvl, n = 8 >> lvl;          // lane distance, elements kept
    const bool up = (fr & m) != 0;
#pragma unroll
    for (int e = 0; e < n; ++e) {
      const float keep = up ? b[e + n] : b[e], send = up ? b[e] : b[e + n];
      const int keepi = up ? bi[e + n] : bi[e], sendi = up ? bi[e] : bi[e + n];
      const float ob = __shfl_xor(send, m);
      const int oi = __shfl_xor(sendi, m);
      const bool take = ob < keep || (ob == keep && oi < keepi);
      b[e] = take ? ob : keep;
      bi[e] = take ? oi : keepi;
    }
  }
  {
    const float ob = __shfl_xor(b[0], 1);
    const int oi = __shfl_xor(bi[0], 1);
    if (ob < b[0] || (ob == b[0] && oi < bi[0])) { b[0] = ob; bi[0] = oi; }
  }
  // the element a lane ends with: bit 3 <- lane bit 4, bit 2 <- bit 3, bit 1 <- bit 2, bit 0 <- bit 1
  const int e_mine = fr >> 1;
  const int64_t t = tok0 + (e_mine & 3) + 8 * (e_mine >> 2) + 4 * fh;
  if ((fr & 1) == 0 && t < n_tokens) {
    pmin[(int64_t)blockIdx.y * n_tokens + t] = b[0];
    pidx[(int64_t)blockIdx.y * n_tokens + t] = bi[0];
  }
}

// The WIDE form of the same search: every code dimension D that is a multiple of 8 up to 256 and has no narrow instantiation (24, 40,
// 48, 56, 72 ... 256).  vq_nearest_mfma_kernel<D> keeps A, two whole B rows and a 64-code tile pair resident, which at D = 256 would be
// over 384 registers of operands and 256 KiB of LDS; here only the A operand is resident (D / 2 registers: the token's components of
// this lane's parity) and B is streamed from LDS in k-chunks of 32 (16 registers per lane, two buffers: the next chunk's 16-byte reads
// are in flight under this chunk's 16 MFMAs; the last chunk may be short, in whole groups of 8 k).  One token / code pair's dot is
// still ONE chain of D / 2 MFMAs onto ONE accumulator, k ascending — the chunks only cut the instruction stream, never the chain —
// so the bits are the oracle's.  D is a template parameter: with `dim` as a kernel argument the chunk and remainder guards became
// scalar branches, one basic block per four MFMAs, and hipcc drained the LDS queue (lgkmcnt(0)) in front of every read: the chain
// waited for each read in turn (8192 x 16384 x 256: 783 us, against 670 us in this form).  Two waves per SIMD are part of the design:
// one wave's single dependent chain does not hold the MFMA rate (the same kernel bounded to one wave per SIMD, reads a whole chunk
// ahead: 873 us; profiles/vq_wide_dims.txt).  Code tiles of 32 (one MFMA block per wave and
// tile), two LDS buffers in the narrow kernel's [code][parity][D / 2] (+ 4 floats) image, the next tile staged through
// ceil(D / 32) float4 registers per thread: thread = (code tid >> 3, pieces tid & 7, + 8, ...).  Rows past the split's end are zeros
// with |e|^2 = +inf, token rows past n_tokens are zeros and store nothing; scan, split merge and grid are the narrow kernel's.
// hipcc's figures for gfx950 (-Rpass-analysis=kernel-resource-usage), __launch_bounds__(256, 2); no AGPRs, no scratch at any D;
// LDS is dynamic, 8 * 32 * (D + 4) + 256 bytes (D = 256 alone passes 64 KiB and takes the opt-in; two blocks still fit a CU):
//     D    VGPRs  waves / SIMD  LDS           D    VGPRs  waves / SIMD  LDS
//     24    103       4          7,424 B      128   168       3         34,048 B
//     56    124       4         15,616 B      136   175       2         36,096 B
//     72    135       3         19,712 B      200   216       2         52,480 B
//     96    148       3         25,856 B      256   247       2         66,816 B
static constexpr int VQ_WIDE_CT = 32;
static constexpr size_t vq_wide_lds_bytes(int dim) { return ((size_t)2 * VQ_WIDE_CT * (dim + 4) + 2 * VQ_WIDE_CT) * sizeof(float); }
// (the dynamic LDS array is declared once, outside the template: the host emulation gives every declaration its own 160 KiB of
// thread-local storage, which 28 instantiations would have multiplied)
__device__ __forceinline__ float* vq_wide_lds() {
  VQ_DYN_LDS(float, lds);
  return lds;
}
template <int D>
__global__ __launch_bounds__(256, 2) void vq_nearest_wide_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                               const float* __restrict__ ee_all, int64_t n_tokens, int n_codes,
                                                               int codes_per_split, float* __restrict__ pmin, int* __restrict__ pidx) {
  constexpr int dim = D, NCH = (D + 31) / 32;         // k-chunks of 32, the last one may be short (whole groups of 8)
  constexpr int CT = VQ_WIDE_CT, KSMAX = 16 * NCH;
  static_assert(CT == 32 && D % 8 == 0 && D >= 8 && D <= 256, "one 32-code MFMA block per tile; 8 threads stage a code");
  float* const lds = vq_wide_lds();                   // tile[2][CT * RS] ([code][parity][KS] + pad), then tee[2][CT]; first, 64 token rows
  static_assert(2 * CT * 4 + 2 * CT >= 64, "64 token rows of dim + 1 floats fit in the tile buffers");
  constexpr int KS = dim >> 1, RS = dim + 4, NQ = dim >> 2;   // RS / 4 is odd: 16 lanes' 16-byte reads cover the 64 banks once
  float* const tee = lds + 2 * CT * RS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int64_t tok0 = (int64_t)blockIdx.x * 128 + wave * 32;
  const int64_t tok = tok0 + fr;
  const bool live = tok < n_tokens;
  // A operand + the token's |z|^2 (full chain, k ascending: both halves of the wave compute it).  The block's 128 token rows come in
  // through the (still unused) tile buffers, 64 rows at a time: one wave instruction copies 256 contiguous bytes of a row, and a
  // lane then walks its own row in LDS (row stride dim + 1, odd: the 32 rows of a wave sit in 32 different banks).  Lanes reading
  // their rows straight from global memory touch 32 cache lines per instruction for 4 bytes each; at 8192 x 1024 x 256 that
  // prologue was most of the kernel's time.
  float az[KSMAX];
  float zz = 0.f;
#pragma unroll
  for (int sidx = 0; sidx < KSMAX; ++sidx) az[sidx] = 0.f;
  {
    constexpr int RZ = dim + 1;
    const int64_t btok0 = (int64_t)blockIdx.x * 128;
#pragma nounroll
    for (int half = 0; half < 2; ++half) {
      if (half) __syncthreads();                       // (the first 64 rows have been read)
#pragma unroll
      for (int kc = 0; kc < (NCH + 1) / 2; ++kc) {       // rows wave, wave + 4, ...: 16 loads in flight per lane
        const int k = kc * 64 + lane;
        if (kc * 64 < dim) {
          float v[16];
#pragma unroll
          for (int rr = 0; rr < 16; ++rr) {
            const int64_t t = btok0 + half * 64 + wave + 4 * rr;
            v[rr] = (t < n_tokens && k < dim) ? z[t * dim + k] : 0.f;
          }
#pragma unroll
          for (int rr = 0; rr < 16; ++rr)
            if (k < dim) lds[(wave + 4 * rr) * RZ + k] = v[rr];
        }
      }
      __syncthreads();
      if ((wave >> 1) == half) {
        const float* zr = lds + ((wave & 1) * 32 + fr) * RZ;
#pragma unroll
        for (int k8 = 0; k8 < KSMAX / 4; ++k8) {
          if (k8 * 8 < dim) {
#pragma unroll
            for (int k = k8 * 8; k < k8 * 8 + 8; ++k) {
              const float v = zr[k];                   // (rows past n_tokens were staged as zeros)
              zz = fmaf(v, v, zz);
              if ((k & 1) == fh) az[k >> 1] = v;
            }
          }
        }
      }
    }
    __syncthreads();                                   // the tiles take the buffers over
  }
  float zzr[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) zzr[e] = __shfl(zz, (e & 3) + 8 * (e >> 2) + 4 * fh);
  const float inf = __uint_as_float(0x7f800000u);
  float best[16];
  int besti[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) { best[e] = inf; besti[e] = 0; }
  const int jbeg = blockIdx.y * codes_per_split;
  int jend = jbeg + codes_per_split;
  if (jend > n_codes) jend = n_codes;
  // tile staging through registers: the next tile's global loads are in flight under this tile's MFMAs
  const int scode = tid >> 3, sq = tid & 7;
  float4 pf[NCH];
  float pe = 0.f;
  auto fetch = [&](int j0) {
    const bool row = j0 + scode < jend;
    const float* src = cb + (int64_t)(row ? j0 + scode : 0) * dim;
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int q = sq + 8 * u;
      pf[u] = (row && q < NQ) ? *(const float4*)(src + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    pe = (tid < CT && j0 + tid < jend) ? ee_all[j0 + tid] : inf;
  };
  auto stash = [&](int buf) {                       // de-interleave: k = 4q, 4q + 2 -> parity 0; 4q + 1, 4q + 3 -> parity 1
    float* dst = lds + (buf * CT + scode) * RS;
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int q = sq + 8 * u;
      if (q < NQ) {
        *(float2*)(dst + 2 * q) = make_float2(pf[u].x, pf[u].z);
        *(float2*)(dst + KS + 2 * q) = make_float2(pf[u].y, pf[u].w);
      }
    }
    if (tid < CT) tee[buf * CT + tid] = pe;
  };
  auto load_b = [&](float (&bz)[16], const float* bsrc, int s0) {   // components s0 ... s0 + 15 of this lane's parity (those below KS)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (s0 + q * 4 < KS) {
        const float4 v = *(const float4*)(bsrc + s0 + q * 4);
        bz[q * 4] = v.x; bz[q * 4 + 1] = v.y; bz[q * 4 + 2] = v.z; bz[q * 4 + 3] = v.w;
      }
    }
  };
  if (jbeg < jend) { fetch(jbeg); stash(0); }
  __syncthreads();
  int buf = 0;
  for (int j0 = jbeg; j0 < jend; j0 += CT, buf ^= 1) {
    const bool more = j0 + CT < jend;
    if (more) fetch(j0 + CT);
    const float* bsrc = lds + (buf * CT + fr) * RS + fh * KS;
    float bz[2][16];
    load_b(bz[0], bsrc, 0);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c * 16 < KS) {
        if (c + 1 < NCH) load_b(bz[(c + 1) & 1], bsrc, (c + 1) * 16);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if (c * 16 + g * 4 < KS) {
#pragma unroll
            for (int sidx = g * 4; sidx < g * 4 + 4; ++sidx) acc = mfma_32x32x2_f32(az[c * 16 + sidx], bz[c & 1][sidx], acc);
          }
        }
      }
    }
    const float ee = tee[buf * CT + fr];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float d = (zzr[e] - 2.f * acc[e]) + ee;
      const bool lt = d < best[e];
      best[e] = lt ? d : best[e];
      besti[e] = lt ? j0 : besti[e];
    }
    if (more) stash(buf ^ 1);                        // (buffer buf ^ 1 was last read one tile ago: behind the barrier below)
    __syncthreads();
  }
  vq_mfma_split_store(best, besti, fr, fh, tok0, n_tokens, pmin, pidx);
}

// |e_j|^2 and the split merge for a `dim` that is a kernel argument (the wide search).  The merge runs one thread per element of
// zq, so that the rows are written coalesced: every thread of a token repeats the (short) scan over the splits.
__global__ __launch_bounds__(256) void vq_code_norms_any_kernel(const float* __restrict__ cb, int n_codes, int dim, float* __restrict__ ee) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_codes) return;
  float acc = 0.f;
#pragma unroll 8
  for (int k = 0; k < dim; ++k) { const float v = cb[(int64_t)j * dim + k]; acc = fmaf(v, v, acc); }
  ee[j] = acc;
}
__global__ __launch_bounds__(256) void vq_finalize_any_kernel(const float* __restrict__ pmin, const int* __restrict__ pidx,
                                                               const float* __restrict__ cb, int64_t n_tokens, int dim, int nsplit,
                                                               int64_t* __restrict__ idx, float* __restrict__ zq, float* __restrict__ min_dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tokens * dim) return;
  const int64_t tok = i / dim;
  const int k = (int)(i - tok * dim);
  float best = pmin[tok];
  int bi = pidx[tok];
  for (int s = 1; s < nsplit; ++s) {
    const float d = pmin[(int64_t)s * n_tokens + tok];
    if (d < best) { best = d; bi = pidx[(int64_t)s * n_tokens + tok]; }
  }
  if (k == 0) {
    idx[tok] = bi;
    if (min_dist) min_dist[tok] = best;
  }
  if (zq) zq[i] = cb[(int64_t)bi * dim + k];
}

template <int D>
__global__ void vq_finalize_kernel(const float* __restrict__ pmin, const int* __restrict__ pidx, const float* __restrict__ cb,
                                   int64_t n_tokens, int nsplit, int64_t* __restrict__ idx, float* __restrict__ zq,
                                   float* __restrict__ min_dist) {
  const int64_t tok = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tok >= n_tokens) return;
  float best = pmin[tok];
  int bi = pidx[tok];
  for (int s = 1; s < nsplit; ++s) {
    const float d = pmin[(int64_t)s * n_tokens + tok];
    if (d < best) { best = d; bi = pidx[(int64_t)s * n_tokens + tok]; }
  }
  idx[tok] = bi;
  if (min_dist) min_dist[tok] = best;
  if (zq)
    for (int k = 0; k < D; ++k) zq[tok * D + k] = cb[(int64_t)bi * D + k];
}

static int vq_nsplit(int64_t n_tokens, int n_codes) {
  const int64_t tb = vq_ceil_div(n_tokens, 256);
  int64_t want = vq_ceil_div(1024, tb);
  const int64_t maxs = vq_ceil_div(n_codes, VQ_TILE);
  if (want > maxs) want = maxs;
  if (want < 1) want = 1;
  return (int)want;
}

static int vq_mfma_blocks() {                      // blocks the fp32-MFMA search aims for
#ifdef VQ_ABLATION_KERNELS                         // (VQ_MFMA_BLOCKS: tools' A/B only — `make ablate` libraries and the emulator)
  static const int v = [] { const char* e = getenv("VQ_MFMA_BLOCKS"); const int x = e ? atoi(e) : 0; return x > 0 ? x : 512; }();
  return v;
#else
  return 512;
#endif
}

extern "C" size_t vq_vq_workspace(int64_t n_tokens, int n_codes) {      // split minima + indices, then the codes' squared norms
  return (size_t)vq_nsplit(n_tokens, n_codes) * (size_t)n_tokens * 8 + (size_t)n_codes * 4 + 64;
}

extern "C" int vq_vq_nearest_fwd(const float* z, const float* codebook, int64_t n_tokens, int n_codes, int dim, int64_t* idx,
                                 float* zq, float* min_dist, void* workspace, size_t ws_bytes, void* stream) {
  VQ_REQUIRE(z && codebook && idx && workspace, VQ_ERR_INVALID, "vq_vq_nearest_fwd: null pointer");
  VQ_REQUIRE(n_tokens > 0 && n_codes > 0, VQ_ERR_INVALID, "vq_vq_nearest_fwd: empty problem");
  VQ_REQUIRE(ws_bytes >= vq_vq_workspace(n_tokens, n_codes), VQ_ERR_WORKSPACE, "vq_vq_nearest_fwd: workspace too small");
  VQ_REQUIRE(dim == 4 || (dim >= 8 && dim <= 256 && dim % 8 == 0), VQ_ERR_UNSUPPORTED,
             "vq_vq_nearest_fwd: unsupported code dim %d (4, or a multiple of 8 from 8 to 256)", dim);
  const int nsplit = vq_nsplit(n_tokens, n_codes);
  float* pmin = (float*)workspace;
  int* pidx = (int*)(pmin + (size_t)nsplit * n_tokens);
  hipStream_t s = (hipStream_t)stream;
  const unsigned fb = (unsigned)vq_ceil_div(n_tokens, 256);
  if (dim == 4) {                                    // the VALU kernel
    const int cps = (int)(vq_ceil_div(vq_ceil_div(n_codes, nsplit), VQ_TILE) * VQ_TILE);
    const int ns = (int)vq_ceil_div(n_codes, cps);
    hipLaunchKernelGGL((vq_nearest_kernel<4>), dim3(fb, ns), dim3(256), 0, s, z, codebook, n_tokens, n_codes, cps, pmin, pidx);
    VQ_CHECK_LAUNCH("vq_vq_nearest_fwd");
    hipLaunchKernelGGL((vq_finalize_kernel<4>), dim3(fb), dim3(256), 0, s, (const float*)pmin, (const int*)pidx, codebook, n_tokens, ns,
                       idx, zq, min_dist);
    VQ_CHECK_LAUNCH("vq_vq_nearest_fwd(finalize)");
    return VQ_OK;
  }
  // every other code dimension on the fp32 MFMA, 128 tokens per block: 8, 16, 32, 64 in vq_nearest_mfma_kernel<D>, the rest in the
  // wide kernel (two blocks per CU — each a long run of code tiles, so the per-block prologue and merge are amortised — and never
  // more splits than the workspace was sized for: its size does not depend on `dim`)
  int64_t msplit = vq_ceil_div(vq_mfma_blocks(), vq_ceil_div(n_tokens, 128));
  if (msplit > nsplit) msplit = nsplit;
  const int mcps = (int)(vq_ceil_div(vq_ceil_div(n_codes, msplit), VQ_TILE) * VQ_TILE);
  const int mns = (int)vq_ceil_div(n_codes, mcps);
  const dim3 mgrid((unsigned)vq_ceil_div(n_tokens, 128), mns);
  float* ee = (float*)(pidx + (size_t)nsplit * n_tokens);
  const dim3 ngrid((unsigned)vq_ceil_div(n_codes, 256));
#define VQ_NM(Dv)                                                                                                  \
  do {                                                                                                             \
    hipLaunchKernelGGL((vq_code_norms_kernel<Dv>), ngrid, dim3(256), 0, s, codebook, n_codes, ee);                 \
    hipLaunchKernelGGL((vq_nearest_mfma_kernel<Dv>), mgrid, dim3(256), 0, s, z, codebook, (const float*)ee, n_tokens, n_codes, mcps, pmin, pidx); \
    VQ_CHECK_LAUNCH("vq_vq_nearest_fwd(mfma)");                                                                    \
    hipLaunchKernelGGL((vq_finalize_kernel<Dv>), dim3(fb), dim3(256), 0, s, (const float*)pmin, (const int*)pidx, codebook, \
                       n_tokens, mns, idx, zq, min_dist);                                                          \
    VQ_CHECK_LAUNCH("vq_vq_nearest_fwd(finalize)");                                                                \
    return VQ_OK;                                                                                                  \
  } while (0)
  if (dim == 32) VQ_NM(32);
  if (dim == 16) VQ_NM(16);
  if (dim == 8) VQ_NM(8);
  if (dim == 64) VQ_NM(64);
#undef VQ_NM
  const size_t lds = vq_wide_lds_bytes(dim);
  static_assert(vq_wide_lds_bytes(248) <= 64 * 1024 && vq_wide_lds_bytes(256) <= 160 * 1024, "only dim 256 needs the LDS opt-in");
  if (lds > 64 * 1024) VQ_RESERVE_LDS(vq_nearest_wide_kernel<256>, vq_wide_lds_bytes(256), "vq_vq_nearest_fwd(wide)");
  hipLaunchKernelGGL(vq_code_norms_any_kernel, ngrid, dim3(256), 0, s, codebook, n_codes, dim, ee);
#define VQ_NW(Dv) \
  case Dv: hipLaunchKernelGGL((vq_nearest_wide_kernel<Dv>), mgrid, dim3(256), lds, s, z, codebook, (const float*)ee, n_tokens, n_codes, mcps, pmin, pidx); break;
  switch (dim) {
    VQ_NW(24) VQ_NW(40) VQ_NW(48) VQ_NW(56) VQ_NW(72) VQ_NW(80) VQ_NW(88) VQ_NW(96) VQ_NW(104) VQ_NW(112) VQ_NW(120) VQ_NW(128)
    VQ_NW(136) VQ_NW(144) VQ_NW(152) VQ_NW(160) VQ_NW(168) VQ_NW(176) VQ_NW(184) VQ_NW(192) VQ_NW(200) VQ_NW(208) VQ_NW(216)
    VQ_NW(224) VQ_NW(232) VQ_NW(240) VQ_NW(248) VQ_NW(256)
  }
#undef VQ_NW
  VQ_CHECK_LAUNCH("vq_vq_nearest_fwd(wide)");
  hipLaunchKernelGGL(vq_finalize_any_kernel, dim3((unsigned)vq_ceil_div(n_tokens * dim, 256)), dim3(256), 0, s, (const float*)pmin,
                     (const int*)pidx, codebook, n_tokens, dim, mns, idx, zq, min_dist);
  VQ_CHECK_LAUNCH("vq_vq_nearest_fwd(finalize)");
  return VQ_OK;
}

// dcodebook[idx_i][:] += gq_i[:]   (fp32 atomics; the summation order of tokens that share a
// code is not fixed — indices, not this gradient, carry the bit-exactness requirement)
// Order-independent (hence deterministic) scatter-add: the contributions are accumulated as 64-bit FIXED-POINT integers — integer
// addition is associative, so the atomics may land in any order — at a power-of-two scale chosen from the measured max |gq| such
// that n_tokens of them cannot overflow 2^60; an fp32 value within 2^-23 of the maximum converts exactly, smaller ones are rounded
// at 2^-47 of the maximum (far below fp32's own resolution of the sum).  fp32 atomics made config 5 the one path of the step
// whose bits depended on the scheduling.
__device__ __forceinline__ double vq_fixed_scale(float amax, int64_t n_tokens) {
  int e_amax = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127 + 1;    // |g| < 2^e_amax
  int lg = 0;
  while (((int64_t)1 << lg) < n_tokens) ++lg;
  int e = 60 - e_amax - lg;
  if (!(amax > 0.f) || e_amax == 129) e = 0;
  if (e > 1000) e = 1000;
  if (e < -1000) e = -1000;
  return ldexp(1.0, e);
}
__global__ __launch_bounds__(256) void vq_scatter_fixed_kernel(const float* __restrict__ gq, const int64_t* __restrict__ idx,
                                                                int64_t n_tokens, int n_codes, int dim,
                                                                const float* __restrict__ amax, unsigned long long* __restrict__ acc) {
  const double scale = vq_fixed_scale(*amax, n_tokens);
  const int64_t total = n_tokens * dim;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / dim;
    const int k = (int)(i - t * dim);
    const int64_t code = idx[t];
    if (code >= 0 && code < n_codes) {
      const long long q = (long long)rint((double)gq[i] * scale);
      atomicAdd(acc + code * dim + k, (unsigned long long)q);              // two's complement: wraps like signed addition
    }
  }
}
__global__ __launch_bounds__(256) void vq_scatter_finish_kernel(const unsigned long long* __restrict__ acc, int64_t n, int64_t n_tokens,
                                                                 const float* __restrict__ amax, float* __restrict__ dcb) {
  const double inv = 1.0 / vq_fixed_scale(*amax, n_tokens);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    dcb[i] += (float)((double)(long long)acc[i] * inv);
}
extern "C" size_t vq_vq_scatter_workspace(int n_codes, int dim) { return (size_t)n_codes * dim * 8 + 64; }
extern "C" int vq_vq_scatter_add(const float* gq, const int64_t* idx, int64_t n_tokens, int n_codes, int dim, float* dcodebook,
                                 void* workspace, size_t ws_bytes, void* stream) {
  VQ_REQUIRE(gq && idx && dcodebook && workspace, VQ_ERR_INVALID, "vq_vq_scatter_add: null pointer");
  VQ_REQUIRE(dim > 0 && n_tokens > 0 && n_codes > 0 && (n_tokens * dim) % 8 == 0, VQ_ERR_INVALID,
             "vq_vq_scatter_add: empty problem, or n_tokens * dim not a multiple of 8");
  VQ_REQUIRE(ws_bytes >= vq_vq_scatter_workspace(n_codes, dim), VQ_ERR_WORKSPACE, "vq_vq_scatter_add: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* amax = (float*)workspace;                                          // [0, 64): the measured max |gq|
  unsigned long long* acc = (unsigned long long*)((char*)workspace + 64);
  hipError_t e = hipMemsetAsync(workspace, 0, vq_vq_scatter_workspace(n_codes, dim), s);
  if (e != hipSuccess) { vq_set_error("vq_vq_scatter_add: hipMemsetAsync: %s", hipGetErrorString(e)); return VQ_ERR_HIP; }
  int rc = vq_absmax(gq, n_tokens * dim, VQ_F32, amax, stream);
  if (rc) return rc;
  int64_t b = vq_ceil_div(n_tokens * dim, 256);
  if (b > 2048) b = 2048;
  hipLaunchKernelGGL(vq_scatter_fixed_kernel, dim3((unsigned)b), dim3(256), 0, s, gq, idx, n_tokens, n_codes, dim, (const float*)amax, acc);
  int64_t b2 = vq_ceil_div((int64_t)n_codes * dim, 256);
  if (b2 > 2048) b2 = 2048;
  hipLaunchKernelGGL(vq_scatter_finish_kernel, dim3((unsigned)b2), dim3(256), 0, s, (const unsigned long long*)acc,
                     (int64_t)n_codes * dim, n_tokens, (const float*)amax, dcodebook);
  VQ_CHECK_LAUNCH("vq_vq_scatter_add");
  return VQ_OK;
}

// ------------------------------------------------------------------------------------------ VQ: EMA codebook
// Exponential-moving-average codebook training (include/vqhip.h "EMA codebook").  The per-step statistics — tokens per
// code and their sums — are accumulated as 64-bit integers (counts) and 64-bit FIXED POINT (sums, vq_fixed_scale as in the scatter-add
// above): integer addition is associative, so the atomics may land in any order AND the partial statistics of several ranks add up
// (an int64 SUM all-reduce) to exactly what one process would have counted over the whole batch.  The update then reads nothing but
// the fp32 state and those integers, in double, and rounds every stored value to fp32 once.
// Accumulator layout (the first 8 * n_codes * (dim + 1) bytes of the workspace — what the host all-reduces): int64 counts [K], then
// int64 sums [K][D]; the update's scratch follows: the unrounded new cluster sizes (double [K]) and 4 doubles per block of 256 codes.
static constexpr int VQ_EMA_BLOCK = 256;
static inline size_t vq_ema_acc_bytes(int n_codes, int dim) { return (size_t)n_codes * ((size_t)dim + 1) * 8; }
extern "C" size_t vq_vq_ema_workspace(int n_codes, int dim) {
  if (n_codes <= 0 || dim <= 0) return 0;
  return vq_ema_acc_bytes(n_codes, dim) + (size_t)n_codes * 8 + (size_t)vq_ceil_div(n_codes, VQ_EMA_BLOCK) * 4 * 8 + 64;
}

// lanes run along `dim`: one wave instruction adds one contiguous segment of 64 / D rows (256 B of a row pair at D = 32)
__global__ __launch_bounds__(256) void vq_ema_accumulate_kernel(const float* __restrict__ tok, const int64_t* __restrict__ idx,
                                                                 int64_t n_tokens, int64_t n_global, int n_codes, int dim,
                                                                 const float* __restrict__ amax, unsigned long long* __restrict__ counts,
                                                                 unsigned long long* __restrict__ sums) {
  const double scale = vq_fixed_scale(*amax, n_global);
  const int64_t total = n_tokens * dim;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / dim;
    const int k = (int)(i - t * dim);
    const int64_t code = idx[t];
    if (code >= 0 && code < n_codes) {
      const long long q = (long long)rint((double)tok[i] * scale);
      atomicAdd(sums + code * dim + k, (unsigned long long)q);               // two's complement: wraps like signed addition
      if (k == 0) atomicAdd(counts + code, 1ull);
    }
  }
}

extern "C" int vq_vq_ema_accumulate(const float* tokens, const int64_t* idx, int64_t n_tokens, int64_t n_global, int n_codes, int dim,
                                    const float* amax, void* workspace, size_t ws_bytes, void* stream) {
  VQ_REQUIRE(tokens && idx && amax && workspace, VQ_ERR_INVALID, "vq_vq_ema_accumulate: null pointer");
  VQ_REQUIRE(n_codes > 0 && dim > 0 && n_tokens > 0 && n_global >= n_tokens, VQ_ERR_INVALID,
             "vq_vq_ema_accumulate: empty problem, or n_global < n_tokens (n_tokens=%lld n_global=%lld n_codes=%d dim=%d)",
             (long long)n_tokens, (long long)n_global, n_codes, dim);
  VQ_REQUIRE(ws_bytes >= vq_vq_ema_workspace(n_codes, dim), VQ_ERR_WORKSPACE, "vq_vq_ema_accumulate: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(workspace, 0, vq_ema_acc_bytes(n_codes, dim), s);
  if (e != hipSuccess) { vq_set_error("vq_vq_ema_accumulate: hipMemsetAsync: %s", hipGetErrorString(e)); return VQ_ERR_HIP; }
  unsigned long long* counts = (unsigned long long*)workspace;
  int64_t b = vq_ceil_div(n_tokens * dim, 256);
  if (b > 2048) b = 2048;
  hipLaunchKernelGGL(vq_ema_accumulate_kernel, dim3((unsigned)b), dim3(256), 0, s, tokens, idx, n_tokens, n_global, n_codes, dim, amax,
                     counts, counts + n_codes);
  VQ_CHECK_LAUNCH("vq_vq_ema_accumulate");
  return VQ_OK;
}

// sum over the block's 256 threads in a FIXED order (a tree over LDS: the same for every launch, block and rank)
__device__ __forceinline__ double vq_ema_block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int o = VQ_EMA_BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  return sh[0];
}
// pass 1, one thread per code: N_k <- g N_k + (1 - g) n_k — stored rounded to fp32, the unrounded value goes on to pass 2 in `nn_out` —
// and the block's partial sums {sum N, sum n, sum n log n, codes with n > 0}
__global__ __launch_bounds__(VQ_EMA_BLOCK) void vq_ema_sizes_kernel(const long long* __restrict__ counts, int n_codes, double decay,
                                                                     float* __restrict__ cluster_size, double* __restrict__ nn_out,
                                                                     double* __restrict__ part) {
  __shared__ double sh[VQ_EMA_BLOCK];
  const int k = blockIdx.x * VQ_EMA_BLOCK + threadIdx.x;
  double nn = 0.0, n = 0.0;
  if (k < n_codes) {
    n = (double)counts[k];
    nn = decay * (double)cluster_size[k] + (1.0 - decay) * n;
    nn_out[k] = nn;
    cluster_size[k] = (float)nn;
  }
  const double s0 = vq_ema_block_sum(nn, sh);
  const double s1 = vq_ema_block_sum(n, sh);
  const double s2 = vq_ema_block_sum(n > 0.0 ? n * log(n) : 0.0, sh);
  const double s3 = vq_ema_block_sum(n > 0.0 ? 1.0 : 0.0, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x * 4] = s0; part[blockIdx.x * 4 + 1] = s1; part[blockIdx.x * 4 + 2] = s2; part[blockIdx.x * 4 + 3] = s3;
  }
}
// pass 2, one thread per codebook element: T = the partials summed in block order (every thread, the same order), then
// m <- g m + (1 - g) s, the smoothed size (N + eps) / (T + K eps) * T and e = m / that — e from the unrounded m
__global__ __launch_bounds__(VQ_EMA_BLOCK) void vq_ema_apply_kernel(const long long* __restrict__ sums, const double* __restrict__ nn_in,
                                                                     const double* __restrict__ part, int n_parts, int n_codes, int dim,
                                                                     int64_t n_global, const float* __restrict__ amax, double decay,
                                                                     double eps, float* __restrict__ embed_sum,
                                                                     float* __restrict__ codebook, float* __restrict__ usage) {
  double T = 0.0, sn = 0.0, snl = 0.0, used = 0.0;
  for (int b = 0; b < n_parts; ++b) { T += part[b * 4]; sn += part[b * 4 + 1]; snl += part[b * 4 + 2]; used += part[b * 4 + 3]; }
  if (blockIdx.x == 0 && threadIdx.x == 0 && usage) {
    // perplexity = exp(-sum p log p), p = n / sum n:  -sum p log p = log(sum n) - (sum n log n) / sum n
    usage[0] = sn > 0.0 ? (float)exp(log(sn) - snl / sn) : 0.f;
    usage[1] = (float)used;
  }
  const double inv = 1.0 / vq_fixed_scale(*amax, n_global);
  const double norm = T / (T + (double)n_codes * eps);
  const int64_t total = (int64_t)n_codes * dim;
  for (int64_t i = (int64_t)blockIdx.x * VQ_EMA_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * VQ_EMA_BLOCK) {
    const int64_t k = i / dim;
    const double m = decay * (double)embed_sum[i] + (1.0 - decay) * ((double)sums[i] * inv);
    const double smoothed = (nn_in[k] + eps) * norm;
    embed_sum[i] = (float)m;
    codebook[i] = (float)(m / smoothed);
  }
}

extern "C" int vq_vq_ema_update(void* workspace, size_t ws_bytes, int64_t n_global, const float* amax, int n_codes, int dim,
                                double decay, double eps, float* cluster_size, float* embed_sum, float* codebook, float* usage,
                                void* stream) {
  VQ_REQUIRE(workspace && amax && cluster_size && embed_sum && codebook, VQ_ERR_INVALID, "vq_vq_ema_update: null pointer");
  VQ_REQUIRE(n_codes > 0 && dim > 0 && n_global > 0, VQ_ERR_INVALID, "vq_vq_ema_update: empty problem (n_codes=%d dim=%d)", n_codes, dim);
  VQ_REQUIRE(decay >= 0.0 && decay <= 1.0 && eps >= 0.0, VQ_ERR_INVALID, "vq_vq_ema_update: decay %g outside [0, 1] or eps %g < 0", decay, eps);
  VQ_REQUIRE(ws_bytes >= vq_vq_ema_workspace(n_codes, dim), VQ_ERR_WORKSPACE, "vq_vq_ema_update: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const long long* counts = (const long long*)workspace;
  const long long* sums = counts + n_codes;
  double* nn = (double*)((char*)workspace + vq_ema_acc_bytes(n_codes, dim));
  double* part = nn + n_codes;
  const int nb = (int)vq_ceil_div(n_codes, VQ_EMA_BLOCK);
  hipLaunchKernelGGL(vq_ema_sizes_kernel, dim3((unsigned)nb), dim3(VQ_EMA_BLOCK), 0, s, counts, n_codes, decay, cluster_size, nn, part);
  VQ_CHECK_LAUNCH("vq_vq_ema_update(sizes)");
  int64_t b2 = vq_ceil_div((int64_t)n_codes * dim, VQ_EMA_BLOCK);
  if (b2 > 2048) b2 = 2048;
  hipLaunchKernelGGL(vq_ema_apply_kernel, dim3((unsigned)b2), dim3(VQ_EMA_BLOCK), 0, s, sums, (const double*)nn, (const double*)part, nb,
                     n_codes, dim, n_global, amax, decay, eps, embed_sum, codebook, usage);
  VQ_CHECK_LAUNCH("vq_vq_ema_update(apply)");
  return VQ_OK;
}

// Reseeding.  The hash (include/vqhip.h): g_k = splitmix64(splitmix64(seed + step) + k) mod n_global.
__host__ __device__ __forceinline__ uint64_t vq_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// phase 0: candidate rows — cand[k] = the token the hash picks for code k if that code is dead (N_k < threshold) AND the token lives on
// this rank ([token_offset, token_offset + n_local) of the global batch), zeros otherwise: summed over ranks, every dead row has
// exactly one non-zero contributor.  (+ 0.f: a token's -0 becomes +0, as the sum over ranks would make it.)
__global__ __launch_bounds__(256) void vq_ema_reseed_pick_kernel(const float* __restrict__ cluster_size, float threshold, uint64_t base,
                                                                  const float* __restrict__ tok, int64_t n_local, int64_t token_offset,
                                                                  int64_t n_global, int n_codes, int dim, float* __restrict__ cand) {
  const int64_t total = (int64_t)n_codes * dim;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t k = i / dim;
    const int d = (int)(i - k * dim);
    float v = 0.f;
    if (cluster_size[k] < threshold) {
      const int64_t g = (int64_t)(vq_splitmix64(base + (uint64_t)k) % (uint64_t)n_global) - token_offset;
      if (g >= 0 && g < n_local) v = tok[g * dim + d] + 0.f;
    }
    cand[i] = v;
  }
}
// phase 1 (after the host's sum over ranks), one thread per codebook element: e_k = m_k = cand[k] for the dead codes, every other row is
// left alone.  N is only READ here (every lane of a row needs the old value); the reset kernel below, one thread per code, follows
// on the same stream and sets N_k = 1 for the same codes.
__global__ __launch_bounds__(256) void vq_ema_reseed_install_kernel(const float* __restrict__ cluster_size, float threshold,
                                                                     const float* __restrict__ cand, int n_codes, int dim,
                                                                     float* __restrict__ embed_sum, float* __restrict__ codebook) {
  const int64_t total = (int64_t)n_codes * dim;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (cluster_size[i / dim] < threshold) {
      const float v = cand[i];
      embed_sum[i] = v;
      codebook[i] = v;
    }
  }
}
__global__ __launch_bounds__(256) void vq_ema_reseed_reset_kernel(float* __restrict__ cluster_size, float threshold, int n_codes) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n_codes && cluster_size[k] < threshold) cluster_size[k] = 1.f;
}

extern "C" int vq_vq_ema_reseed(int phase, float* cluster_size, float threshold, int64_t step, uint64_t seed, const float* tokens,
                                int64_t n_local, int64_t token_offset, int64_t n_global, int n_codes, int dim, float* candidates,
                                float* embed_sum, float* codebook, void* stream) {
  VQ_REQUIRE(phase == 0 || phase == 1, VQ_ERR_INVALID, "vq_vq_ema_reseed: phase %d (0 = pick, 1 = install)", phase);
  VQ_REQUIRE(cluster_size && candidates, VQ_ERR_INVALID, "vq_vq_ema_reseed: null pointer");
  VQ_REQUIRE(n_codes > 0 && dim > 0, VQ_ERR_INVALID, "vq_vq_ema_reseed: empty problem (n_codes=%d dim=%d)", n_codes, dim);
  hipStream_t s = (hipStream_t)stream;
  if (phase == 0) {
    VQ_REQUIRE(tokens, VQ_ERR_INVALID, "vq_vq_ema_reseed: null pointer (tokens)");
    VQ_REQUIRE(n_local > 0 && token_offset >= 0 && n_global >= token_offset + n_local && step >= 0, VQ_ERR_INVALID,
               "vq_vq_ema_reseed: tokens [%lld, %lld + %lld) outside the global batch of %lld, or step < 0", (long long)token_offset,
               (long long)token_offset, (long long)n_local, (long long)n_global);
    int64_t b = vq_ceil_div((int64_t)n_codes * dim, 256);
    if (b > 2048) b = 2048;
    const uint64_t base = vq_splitmix64(seed + (uint64_t)step);
    hipLaunchKernelGGL(vq_ema_reseed_pick_kernel, dim3((unsigned)b), dim3(256), 0, s, (const float*)cluster_size, threshold, base, tokens,
                       n_local, token_offset, n_global, n_codes, dim, candidates);
    VQ_CHECK_LAUNCH("vq_vq_ema_reseed(pick)");
    return VQ_OK;
  }
  VQ_REQUIRE(embed_sum && codebook, VQ_ERR_INVALID, "vq_vq_ema_reseed: null pointer (embed_sum / codebook)");
  int64_t b1 = vq_ceil_div((int64_t)n_codes * dim, 256);
  if (b1 > 2048) b1 = 2048;
  hipLaunchKernelGGL(vq_ema_reseed_install_kernel, dim3((unsigned)b1), dim3(256), 0, s, (const float*)cluster_size, threshold,
                     (const float*)candidates, n_codes, dim, embed_sum, codebook);
  hipLaunchKernelGGL(vq_ema_reseed_reset_kernel, dim3((unsigned)vq_ceil_div(n_codes, 256)), dim3(256), 0, s, cluster_size, threshold,
                     n_codes);
  VQ_CHECK_LAUNCH("vq_vq_ema_reseed(install)");
  return VQ_OK;
}
