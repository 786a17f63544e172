// SASRec: a causal self-attention encoder between the history gather and model_output, over hist [Hn, T, C] (C = Di + Dc,
// histories left aligned, len = seq_len clamped to 0 .. T valid steps each, dh = C / nheads):
//
//   x_0[t] = hist[t] + pos[len - 1 - t]                                   (position counted back from the most recent action)
//   block l:  u = LN1(x)        q, k, v = u Wq + bq, u Wk + bk, u Wv + bv
//             a[t, s] = softmax over s <= t of q_h[t] . k_h[s] / sqrt(dh)    o[t] = concat_h sum_s a_h[t, s] v_h[s]
//             y = x + o Wo + bo     w = LN2(y)     x' = y + relu(w W1 + b1) W2 + b2
//   s = LNf(x_L[len - 1])
//   LN(v) = gamma * (v - mean) / sqrt(var + 1e-8) + beta over the channel axis, biased variance; relu open for > 0 only.
//
// Steps t >= len are padding: never a key (a valid query t < len only sees s <= t < len), never a query, zero gradient.
// len = 0: s = 0 and no gradient.
//
// Parameter block (floats; the order the variables are created in, each contiguous; every matrix is [in][out]):
//   pos [Tmax][C] | per block: gamma1 [C] | beta1 [C] | Wq [C][C] | bq [C] | Wk | bk | Wv | bv | Wo | bo | gamma2 | beta2 |
//   W1 [C][C] | b1 [C] | W2 [C][C] | b2 [C] | ... | gammaf [C] | betaf [C]
// = Tmax C + nblocks (6 C^2 + 10 C) + 2 C floats; C is a multiple of 8, so every tensor starts 16-byte aligned and the block
// has no padding.  The gradient block (a row of partial sums) has the same layout.
//
// Work split: a workgroup of 256 threads owns a SLICE of S = min(256 / T, what LDS holds) histories at a time and walks
// slices in a persistent loop; thread s * T + t owns position t of the slice's history s, as a query and as a key.  A
// history's activations stay in LDS from block to block (row stride C + 1 words: a wave's 64 rows hit 64 banks); weights
// are read at wave-uniform addresses.  fp32 FMA chains in a fixed order per output element.  The softmax runs in the
// query's thread over its keys, two passes (maximum, then sum and weighted values): no [T, T] scores anywhere.
//   forward   LDS per history: 5 T (C + 1) words (x, q, k, v, o).
//   backward  LDS per history: 9 T (C + 1) + T (C / 2 + 1) words (x, xhat2, q, k, v, o, the gradient, two scratch rows;
//             log-sum-exp and sum a da per head), plus S + 1 words.  It recomputes a block from its saved input x_l (the
//             training state: every block's input and the one row x_L[len - 1] per history), then walks it backwards.  The
//             attention backward is a gather: the query's thread sums dq over its keys, the key's thread sums dk and dv
//             over the queries t >= s from q, dO, the log-sum-exp and sum a da.  Dense gradients are summed over the
//             slice's valid rows by one owner thread per element into the workgroup's row of partial sums; the caller
//             reduces the rows in ascending order.  No atomics: two runs are bit-identical.
// Both kernels opt into up to 160 KB of LDS per workgroup (clsr_sasrec_supported says so for the backward, the larger).
#include "common.h"

#define SA_THREADS 256
#define SA_LDS_FLOATS 40960          // 160 KB per workgroup
#define SA_MAX_C 64
#define SA_MAX_BLOCKS 4
#define SA_MAX_T 256
#define SA_MAX_PARTS 512
#define SA_WS_FLOATS (1L << 24)
#define SA_EPS 1e-8f

__host__ __device__ static inline long sa_block_floats(int C) { return 6L * C * C + 10L * C; }
static inline long sa_fwd_hist_floats(int T, int C) { return 5L * T * (C + 1); }
static inline long sa_bwd_hist_floats(int T, int C) { return 9L * T * (C + 1) + (long)T * (C / 2 + 1); }
static inline long sa_fixed_floats(int S) { return S + 1; }

static int sa_slice(int T, int C, int training) {
  const long per = (training ? sa_bwd_hist_floats(T, C) : sa_fwd_hist_floats(T, C)) + 1;
  long s = (SA_LDS_FLOATS - 1) / per;
  if (s > SA_THREADS / T) s = SA_THREADS / T;
  return (int)s;
}

static int sa_dims_ok(int T, int C) { return T > 0 && T <= SA_MAX_T && C > 0 && C % 8 == 0 && C <= SA_MAX_C; }

extern "C" int clsr_sasrec_max_channels(void) { return SA_MAX_C; }
extern "C" int clsr_sasrec_max_blocks(void) { return SA_MAX_BLOCKS; }
extern "C" int clsr_sasrec_max_steps(void) { return SA_MAX_T; }
extern "C" int clsr_sasrec_max_parts(void) { return SA_MAX_PARTS; }
extern "C" long clsr_sasrec_lds_budget_bytes(void) { return 4L * SA_LDS_FLOATS; }

// LDS bytes of a slice of ONE history (training: the backward, which is the larger)
extern "C" long clsr_sasrec_lds_bytes(int T, int C, int training) {
  if (T <= 0 || C <= 0) return 0;
  return 4L * ((training ? sa_bwd_hist_floats(T, C) : sa_fwd_hist_floats(T, C)) + sa_fixed_floats(1));
}

extern "C" int clsr_sasrec_supported(int T, int Tmax, int C, int nblocks, int nheads) {
  if (!sa_dims_ok(T, C) || Tmax < T || Tmax > SA_MAX_T) return 0;
  if (nblocks < 1 || nblocks > SA_MAX_BLOCKS || nheads < 1 || C % nheads || (C / nheads) % 4) return 0;
  return clsr_sasrec_lds_bytes(T, C, 1) <= clsr_sasrec_lds_budget_bytes();
}

extern "C" long clsr_sasrec_param_floats(int Tmax, int C, int nblocks) {
  if (C <= 0 || C % 8 || Tmax < 1 || nblocks < 1) return 0;
  return (long)Tmax * C + nblocks * sa_block_floats(C) + 2L * C;
}

// floats of the training state: every block's input [nblocks][Hn][T][C], then x_L[len - 1] [Hn][C]
extern "C" long clsr_sasrec_saved_floats(long Hn, int T, int C, int nblocks) {
  if (Hn <= 0 || T <= 0 || C <= 0 || nblocks < 1) return 0;
  return (long)nblocks * Hn * T * C + Hn * C;
}

// histories a workgroup holds at a time (training: the backward)
extern "C" int clsr_sasrec_slice(int T, int C, int training) {
  if (!sa_dims_ok(T, C)) return 0;
  return sa_slice(T, C, training);
}

// workgroups of the backward = rows of partial sums
extern "C" int clsr_sasrec_parts(long Hn, int T, int Tmax, int C, int nblocks) {
  if (Hn <= 0 || !clsr_sasrec_supported(T, Tmax, C, nblocks, 1)) return 0;
  const int S = sa_slice(T, C, 1);
  long parts = (Hn + S - 1) / S;
  if (parts > SA_MAX_PARTS) parts = SA_MAX_PARTS;
  const long cap = SA_WS_FLOATS / clsr_sasrec_param_floats(Tmax, C, nblocks);
  if (parts > cap) parts = cap;
  return parts < 1 ? 1 : (int)parts;
}

extern "C" long clsr_sasrec_workspace_floats(long Hn, int T, int Tmax, int C, int nblocks) {
  return clsr_sasrec_parts(Hn, T, Tmax, C, nblocks) * clsr_sasrec_param_floats(Tmax, C, nblocks);
}

// ------------------------------------------------------------------------------------------------ device helpers
struct SaOff {
  int g1, be1, Wq, bq, Wk, bk, Wv, bv, Wo, bo, g2, be2, W1, b1, W2, b2;
};
__device__ __forceinline__ SaOff sa_offsets(int C) {
  const int m = C * C + C;
  SaOff o;
  o.g1 = 0;
  o.be1 = C;
  o.Wq = 2 * C;
  o.bq = o.Wq + C * C;
  o.Wk = o.Wq + m;
  o.bk = o.Wk + C * C;
  o.Wv = o.Wk + m;
  o.bv = o.Wv + C * C;
  o.Wo = o.Wv + m;
  o.bo = o.Wo + C * C;
  o.g2 = o.Wo + m;
  o.be2 = o.g2 + C;
  o.W1 = o.be2 + C;
  o.b1 = o.W1 + C * C;
  o.W2 = o.W1 + m;
  o.b2 = o.W2 + C * C;
  return o;
}

// mean and 1 / sqrt(biased variance + eps) of v[0 .. n)
__device__ __forceinline__ void sa_stats(const float* v, int n, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll 4
  for (int i = 0; i < n; ++i) s += v[i];
  mean = s / (float)n;
  float q = 0.f;
#pragma unroll 4
  for (int i = 0; i < n; ++i) {
    const float d = v[i] - mean;
    q = fmaf(d, d, q);
  }
  rstd = 1.0f / sqrtf(q / (float)n + SA_EPS);
}

// acc[q] += sum_n v[n] * W[n * ld + q], n < N (W: wave-uniform address)
__device__ __forceinline__ void sa_axpy4(const float* v, const float* __restrict__ W, int ld, int N, f32x4& acc) {
#pragma unroll 4
  for (int n = 0; n < N; ++n) {
    const float x = v[n];
    const f32x4 w = ld4(W + (long)n * ld);
    acc.x = fmaf(x, w.x, acc.x);
    acc.y = fmaf(x, w.y, acc.y);
    acc.z = fmaf(x, w.z, acc.z);
    acc.w = fmaf(x, w.w, acc.w);
  }
}

// acc[q] += sum_n (g[n] * v[n] + b[n]) * W[n * ld + q]: a layer norm's output formed on the way (v holds xhat)
__device__ __forceinline__ void sa_axpy4_ln(const float* v, const float* __restrict__ g, const float* __restrict__ b,
                                            const float* __restrict__ W, int ld, int N, f32x4& acc) {
#pragma unroll 4
  for (int n = 0; n < N; ++n) {
    const float x = fmaf(g[n], v[n], b[n]);
    const f32x4 w = ld4(W + (long)n * ld);
    acc.x = fmaf(x, w.x, acc.x);
    acc.y = fmaf(x, w.y, acc.y);
    acc.z = fmaf(x, w.z, acc.z);
    acc.w = fmaf(x, w.w, acc.w);
  }
}

// acc[q] += sum_n v[n] * W[q * ld + n], n < N (a multiple of 4)
__device__ __forceinline__ void sa_dot4(const float* v, const float* __restrict__ W, int ld, int N, f32x4& acc) {
#pragma unroll 2
  for (int n = 0; n < N; n += 4) {
    const float x0 = v[n], x1 = v[n + 1], x2 = v[n + 2], x3 = v[n + 3];
    const f32x4 w0 = ld4(W + n), w1 = ld4(W + ld + n), w2 = ld4(W + 2 * ld + n), w3 = ld4(W + 3 * ld + n);
    acc.x = fmaf(x3, w0.w, fmaf(x2, w0.z, fmaf(x1, w0.y, fmaf(x0, w0.x, acc.x))));
    acc.y = fmaf(x3, w1.w, fmaf(x2, w1.z, fmaf(x1, w1.y, fmaf(x0, w1.x, acc.y))));
    acc.z = fmaf(x3, w2.w, fmaf(x2, w2.z, fmaf(x1, w2.y, fmaf(x0, w2.x, acc.z))));
    acc.w = fmaf(x3, w3.w, fmaf(x2, w3.z, fmaf(x1, w3.y, fmaf(x0, w3.x, acc.w))));
  }
}

__device__ __forceinline__ float sa_relu(float v) { return v > 0.f ? v : 0.f; }

__device__ __forceinline__ float sa_dot(const float* a, const float* b, int n) {
  float s = 0.f;
#pragma unroll 4
  for (int i = 0; i < n; ++i) s = fmaf(a[i], b[i], s);
  return s;
}

// the lengths of a slice's histories, clamped to 0 .. T, into slen
__device__ __forceinline__ void sa_lens(const int* __restrict__ seq_len, int len_stride, long base, int nact, int T,
                                        int* slen) {
  for (int s = threadIdx.x; s < nact; s += SA_THREADS) {
    const int n = seq_len[(base + s) * len_stride];
    slen[s] = n < 0 ? 0 : (n > T ? T : n);
  }
}

// q, k, v of the thread's row from xhat1 on the way (xr raw, mean / rstd of it), into qr, kr, vr
__device__ __forceinline__ void sa_qkv(const float* xr, float mean, float rstd, float* tmp, const float* __restrict__ p,
                                       const SaOff& of, int C, float* qr, float* kr, float* vr) {
  // tmp (the row of o, not yet in use) holds xhat1 while the three products read it
  for (int c = 0; c < C; ++c) tmp[c] = (xr[c] - mean) * rstd;
  for (int o = 0; o < C; o += 4) {
    f32x4 aq = ld4(p + of.bq + o), ak = ld4(p + of.bk + o), av = ld4(p + of.bv + o);
    sa_axpy4_ln(tmp, p + of.g1, p + of.be1, p + of.Wq + o, C, C, aq);
    sa_axpy4_ln(tmp, p + of.g1, p + of.be1, p + of.Wk + o, C, C, ak);
    sa_axpy4_ln(tmp, p + of.g1, p + of.be1, p + of.Wv + o, C, C, av);
    qr[o] = aq.x, qr[o + 1] = aq.y, qr[o + 2] = aq.z, qr[o + 3] = aq.w;
    kr[o] = ak.x, kr[o + 1] = ak.y, kr[o + 2] = ak.z, kr[o + 3] = ak.w;
    vr[o] = av.x, vr[o + 1] = av.y, vr[o + 2] = av.z, vr[o + 3] = av.w;
  }
}

// the attention of query row t over the keys 0 .. t of its history (K0 / V0: row 0 of the history), into orow; the
// log-sum-exp of every head into lse (NULL: not wanted)
__device__ __forceinline__ void sa_attend(const float* qr, const float* K0, const float* V0, int LX, int t, int nh, int dh,
                                          float scale, float* orow, float* lse) {
  for (int hd = 0; hd < nh; ++hd) {
    const int c0 = hd * dh;
    float m = -INFINITY;
    for (int s = 0; s <= t; ++s) m = fmaxf(m, sa_dot(qr + c0, K0 + s * LX + c0, dh) * scale);
    for (int d = 0; d < dh; ++d) orow[c0 + d] = 0.f;
    float l = 0.f;
    for (int s = 0; s <= t; ++s) {
      const float e = expf(sa_dot(qr + c0, K0 + s * LX + c0, dh) * scale - m);
      l += e;
      const float* vs = V0 + s * LX + c0;
      for (int d = 0; d < dh; ++d) orow[c0 + d] = fmaf(e, vs[d], orow[c0 + d]);
    }
    const float inv = 1.0f / l;
    for (int d = 0; d < dh; ++d) orow[c0 + d] *= inv;
    if (lse) lse[hd] = m + logf(l);
  }
}

// ------------------------------------------------------------------------------------------------ forward
// saved (training; NULL: scoring): every block's input [nb][Hn][T][C] (padding rows zero), then x_L[len - 1] [Hn][C].
// out: s into rows h rep + g, g < rep, ldo floats apart, columns 0 .. C.
__global__ void __launch_bounds__(SA_THREADS) sa_fwd_kernel(const float* __restrict__ hist, const int* __restrict__ seq_len,
                                                            int len_stride, long Hn, int T, int C,
                                                            const float* __restrict__ params, int Tmax, int nb, int nh,
                                                            float* __restrict__ saved, float* __restrict__ out, int ldo,
                                                            int rep, int S) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, LX = C + 1, dh = C / nh;
  float* X = lds;
  float* Q = X + S * T * LX;
  float* K = Q + S * T * LX;
  float* V = K + S * T * LX;
  float* O = V + S * T * LX;
  int* slen = reinterpret_cast<int*>(O + S * T * LX);
  const SaOff of = sa_offsets(C);
  const long PB = sa_block_floats(C);
  const float* __restrict__ pos = params;
  const float* __restrict__ blocks = params + (long)Tmax * C;
  const float* __restrict__ fin = blocks + nb * PB;
  const float scale = 1.0f / sqrtf((float)dh);
  const int t = tid % T, hs = tid / T;
  for (long base = (long)blockIdx.x * S; base < Hn; base += (long)gridDim.x * S) {
    const int nact = (int)min((long)S, Hn - base), rows = nact * T;
    __syncthreads();
    sa_lens(seq_len, len_stride, base, nact, T, slen);
    __syncthreads();
    {
      const float* __restrict__ src = hist + base * T * C;
      for (int e = tid; e < rows * C; e += SA_THREADS) {
        const int r = e / C, c = e - r * C, h = r / T, tt = r - h * T, n = slen[h];
        X[r * LX + c] = tt < n ? src[e] + pos[(n - 1 - tt) * C + c] : 0.f;
      }
    }
    __syncthreads();
    const int len = tid < rows ? slen[hs] : 0;
    const bool active = tid < rows && t < len;
    const int row = active ? tid : 0;
    float* xr = X + row * LX;
    float* qr = Q + row * LX;
    float* kr = K + row * LX;
    float* vr = V + row * LX;
    float* orow = O + row * LX;
    for (int l = 0; l < nb; ++l) {
      const float* __restrict__ p = blocks + l * PB;
      if (saved) {
        float* __restrict__ dst = saved + ((long)l * Hn + base) * T * C;
        for (int e = tid; e < rows * C; e += SA_THREADS) {
          const int r = e / C;
          dst[e] = X[r * LX + (e - r * C)];
        }
      }
      if (active) {
        float mean, rstd;
        sa_stats(xr, C, mean, rstd);
        sa_qkv(xr, mean, rstd, orow, p, of, C, qr, kr, vr);
      }
      __syncthreads();
      if (active) {
        sa_attend(qr, K + hs * T * LX, V + hs * T * LX, LX, t, nh, dh, scale, orow, nullptr);
        for (int o = 0; o < C; o += 4) {
          f32x4 acc = ld4(p + of.bo + o);
          sa_axpy4(orow, p + of.Wo + o, C, C, acc);
          xr[o] += acc.x, xr[o + 1] += acc.y, xr[o + 2] += acc.z, xr[o + 3] += acc.w;
        }
        float mean, rstd;
        sa_stats(xr, C, mean, rstd);
        for (int c = 0; c < C; ++c) orow[c] = (xr[c] - mean) * rstd;
        for (int o = 0; o < C; o += 4) {
          f32x4 acc = ld4(p + of.b1 + o);
          sa_axpy4_ln(orow, p + of.g2, p + of.be2, p + of.W1 + o, C, C, acc);
          qr[o] = sa_relu(acc.x), qr[o + 1] = sa_relu(acc.y), qr[o + 2] = sa_relu(acc.z), qr[o + 3] = sa_relu(acc.w);
        }
        for (int o = 0; o < C; o += 4) {
          f32x4 acc = ld4(p + of.b2 + o);
          sa_axpy4(qr, p + of.W2 + o, C, C, acc);
          xr[o] += acc.x, xr[o + 1] += acc.y, xr[o + 2] += acc.z, xr[o + 3] += acc.w;
        }
      }
      __syncthreads();      // (the next block's k and v overwrite rows that other queries have just read)
    }
    // ---- s = LNf(x_L[len - 1]) (len = 0: zeros), once per row of the history group
    if (tid < rows && t == (len > 0 ? len - 1 : 0)) {
      const long h = base + hs;
      float mean = 0.f, rstd = 0.f;
      if (len > 0) sa_stats(xr, C, mean, rstd);
      if (saved) {
        float* __restrict__ dst = saved + (long)nb * Hn * T * C + h * C;
        for (int c = 0; c < C; ++c) dst[c] = len > 0 ? xr[c] : 0.f;
      }
      for (int c = 0; c < C; ++c) {
        const float v = len > 0 ? fmaf(fin[c], (xr[c] - mean) * rstd, fin[C + c]) : 0.f;
        for (int g = 0; g < rep; ++g) out[(h * rep + g) * ldo + c] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
__device__ __forceinline__ void sa_acc(float* __restrict__ g, bool first, float v) { *g = first ? v : *g + v; }

// gp[e] (+)= sum over the slice's valid rows r of A(r, e / C) * Bm[r][e % C], e < C * C (one owner thread per element, rows
// ascending); LN: A = g[i] * Am[r][i] + b[i] (a layer norm's output from xhat), else A = Am[r][i].  Then the column sums
// of Bm into gb (NULL: none).
template <bool LN>
__device__ __forceinline__ void sa_dw(const float* Am, const float* Bm, const float* __restrict__ g,
                                      const float* __restrict__ b, int LX, int C, int T, int nact, const int* slen,
                                      float* __restrict__ gp, float* __restrict__ gb, bool first) {
  for (int e = threadIdx.x; e < C * C; e += SA_THREADS) {
    const int i = e / C, o = e - i * C;
    const float gi = LN ? g[i] : 1.f, bi = LN ? b[i] : 0.f;
    float s = 0.f;
    for (int h = 0; h < nact; ++h)
      for (int r = h * T, re = h * T + slen[h]; r < re; ++r)
        s = fmaf(LN ? fmaf(gi, Am[r * LX + i], bi) : Am[r * LX + i], Bm[r * LX + o], s);
    sa_acc(gp + e, first, s);
  }
  if (gb)
    for (int o = threadIdx.x; o < C; o += SA_THREADS) {
      float s = 0.f;
      for (int h = 0; h < nact; ++h)
        for (int r = h * T, re = h * T + slen[h]; r < re; ++r) s += Bm[r * LX + o];
      sa_acc(gb + o, first, s);
    }
}

// d gamma[c] (+)= sum_r Dm[r][c] * Xh[r][c], d beta[c] (+)= sum_r Dm[r][c] over the slice's valid rows
__device__ __forceinline__ void sa_dln(const float* Dm, const float* Xh, int LX, int C, int T, int nact, const int* slen,
                                       float* __restrict__ gg, float* __restrict__ gb, bool first) {
  for (int c = threadIdx.x; c < C; c += SA_THREADS) {
    float sg = 0.f, sb = 0.f;
    for (int h = 0; h < nact; ++h)
      for (int r = h * T, re = h * T + slen[h]; r < re; ++r) {
        const float d = Dm[r * LX + c];
        sg = fmaf(d, Xh[r * LX + c], sg);
        sb += d;
      }
    sa_acc(gg + c, first, sg);
    sa_acc(gb + c, first, sb);
  }
}

// gr += the layer norm's backward of du (the gradient w.r.t. its output) at xhat, gain g
__device__ __forceinline__ void sa_ln_bwd(const float* du, const float* xh, const float* __restrict__ g, float rstd, int C,
                                          float* gr) {
  float s1 = 0.f, s2 = 0.f;
  for (int c = 0; c < C; ++c) {
    const float dx = du[c] * g[c];
    s1 += dx;
    s2 = fmaf(dx, xh[c], s2);
  }
  s1 /= (float)C, s2 /= (float)C;
  for (int c = 0; c < C; ++c) gr[c] += rstd * (du[c] * g[c] - s1 - xh[c] * s2);
}

__global__ void __launch_bounds__(SA_THREADS) sa_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ saved,
                                                            const int* __restrict__ seq_len, int len_stride, long Hn,
                                                            int T, int C, const float* __restrict__ params, int Tmax,
                                                            int nb, int nh, float* __restrict__ dhist,
                                                            float* __restrict__ partial, int S) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, LX = C + 1, LS = C / 2 + 1, dh = C / nh;
  const int BUF = S * T * LX;
  float* X = lds;             // the block's input x_l
  float* Y = X + BUF;         // xhat2, then d v
  float* Q = Y + BUF;         // q, then d u
  float* K = Q + BUF;
  float* V = K + BUF;
  float* O = V + BUF;         // o, then d q
  float* G = O + BUF;         // gradient w.r.t. the block's output, then its input
  float* T1 = G + BUF;        // d h1, then d o, then xhat1
  float* H1 = T1 + BUF;       // h1, then d w, then d k
  float* ST = H1 + BUF;       // per row: log-sum-exp [nh] | sum a da [nh]
  int* slen = reinterpret_cast<int*>(ST + S * T * LS);
  const SaOff of = sa_offsets(C);
  const long PB = sa_block_floats(C);
  const float* __restrict__ blocks = params + (long)Tmax * C;
  const float* __restrict__ fin = blocks + nb * PB;
  const float scale = 1.0f / sqrtf((float)dh);
  const int t = tid % T, hs = tid / T;
  float* __restrict__ part = partial + (long)blockIdx.x * ((long)Tmax * C + nb * PB + 2 * C);
  float* __restrict__ part_blocks = part + (long)Tmax * C;
  float* __restrict__ part_fin = part_blocks + nb * PB;
  const float* __restrict__ xlast = saved + (long)nb * Hn * T * C;
  bool first = true;
  for (long base = (long)blockIdx.x * S; base < Hn; base += (long)gridDim.x * S, first = false) {
    const int nact = (int)min((long)S, Hn - base), rows = nact * T;
    __syncthreads();
    sa_lens(seq_len, len_stride, base, nact, T, slen);
    for (int e = tid; e < rows * LX; e += SA_THREADS) G[e] = 0.f;
    __syncthreads();
    const int len = tid < rows ? slen[hs] : 0;
    const bool active = tid < rows && t < len;
    const int row = active ? tid : 0;
    float* xr = X + row * LX;
    float* yr = Y + row * LX;
    float* qr = Q + row * LX;
    float* kr = K + row * LX;
    float* vr = V + row * LX;
    float* orow = O + row * LX;
    float* gr = G + row * LX;
    float* t1 = T1 + row * LX;
    float* h1 = H1 + row * LX;
    float* st = ST + row * LS;
    const float* K0 = K + hs * T * LX;
    const float* V0 = V + hs * T * LX;
    // ---- the final layer norm: xhatf of x_L[len - 1] -> T1, its backward -> G (row len - 1 only)
    if (active && t == len - 1) {
      const float* __restrict__ xl = xlast + (base + hs) * C;
      const float* __restrict__ ds = dout + (base + hs) * C;
      for (int c = 0; c < C; ++c) t1[c] = xl[c];
      float mean, rstd;
      sa_stats(t1, C, mean, rstd);
      for (int c = 0; c < C; ++c) t1[c] = (t1[c] - mean) * rstd, h1[c] = ds[c];
      sa_ln_bwd(h1, t1, fin, rstd, C, gr);
    }
    __syncthreads();
    for (int c = tid; c < C; c += SA_THREADS) {
      float sg = 0.f, sb = 0.f;
      for (int h = 0; h < nact; ++h)
        if (slen[h] > 0) {
          const int r = h * T + slen[h] - 1;
          sg = fmaf(H1[r * LX + c], T1[r * LX + c], sg);
          sb += H1[r * LX + c];
        }
      sa_acc(part_fin + c, first, sg);
      sa_acc(part_fin + C + c, first, sb);
    }
    for (int l = nb - 1; l >= 0; --l) {
      const float* __restrict__ p = blocks + l * PB;
      float* __restrict__ gp = part_blocks + l * PB;
      __syncthreads();
      {
        const float* __restrict__ src = saved + ((long)l * Hn + base) * T * C;
        for (int e = tid; e < rows * C; e += SA_THREADS) {
          const int r = e / C;
          X[r * LX + (e - r * C)] = src[e];
        }
      }
      __syncthreads();
      // ---- the block again: q, k, v
      float mean1 = 0.f, rstd1 = 0.f, rstd2 = 0.f;
      if (active) {
        sa_stats(xr, C, mean1, rstd1);
        sa_qkv(xr, mean1, rstd1, orow, p, of, C, qr, kr, vr);
      }
      __syncthreads();
      // ---- o and the log-sum-exp, xhat2 -> Y, h1 -> H1, then d h1 = gate (G . W2^T) -> T1
      if (active) {
        sa_attend(qr, K0, V0, LX, t, nh, dh, scale, orow, st);
        for (int o = 0; o < C; o += 4) {
          f32x4 acc = ld4(p + of.bo + o);
          sa_axpy4(orow, p + of.Wo + o, C, C, acc);
          yr[o] = xr[o] + acc.x, yr[o + 1] = xr[o + 1] + acc.y, yr[o + 2] = xr[o + 2] + acc.z, yr[o + 3] = xr[o + 3] + acc.w;
        }
        float mean2;
        sa_stats(yr, C, mean2, rstd2);
        for (int c = 0; c < C; ++c) yr[c] = (yr[c] - mean2) * rstd2;
        for (int o = 0; o < C; o += 4) {
          f32x4 acc = ld4(p + of.b1 + o);
          sa_axpy4_ln(yr, p + of.g2, p + of.be2, p + of.W1 + o, C, C, acc);
          h1[o] = sa_relu(acc.x), h1[o + 1] = sa_relu(acc.y), h1[o + 2] = sa_relu(acc.z), h1[o + 3] = sa_relu(acc.w);
        }
        for (int j = 0; j < C; j += 4) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          sa_dot4(gr, p + of.W2 + j * C, C, C, acc);
          t1[j] = h1[j] > 0.f ? acc.x : 0.f, t1[j + 1] = h1[j + 1] > 0.f ? acc.y : 0.f;
          t1[j + 2] = h1[j + 2] > 0.f ? acc.z : 0.f, t1[j + 3] = h1[j + 3] > 0.f ? acc.w : 0.f;
        }
      }
      __syncthreads();
      // ---- d W2, d b2, d W1, d b1
      sa_dw<false>(H1, G, nullptr, nullptr, LX, C, T, nact, slen, gp + of.W2, gp + of.b2, first);
      sa_dw<true>(Y, T1, p + of.g2, p + of.be2, LX, C, T, nact, slen, gp + of.W1, gp + of.b1, first);
      __syncthreads();
      // ---- d w = d h1 . W1^T -> H1; G += LN2 backward: G is d y
      if (active) {
        for (int c = 0; c < C; c += 4) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          sa_dot4(t1, p + of.W1 + c * C, C, C, acc);
          h1[c] = acc.x, h1[c + 1] = acc.y, h1[c + 2] = acc.z, h1[c + 3] = acc.w;
        }
        sa_ln_bwd(h1, yr, p + of.g2, rstd2, C, gr);
        // ---- d o = d y . Wo^T -> T1; sum a da per head = d o . o
        for (int c = 0; c < C; c += 4) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          sa_dot4(gr, p + of.Wo + c * C, C, C, acc);
          t1[c] = acc.x, t1[c + 1] = acc.y, t1[c + 2] = acc.z, t1[c + 3] = acc.w;
        }
        for (int hd = 0; hd < nh; ++hd) st[nh + hd] = sa_dot(t1 + hd * dh, orow + hd * dh, dh);
      }
      __syncthreads();
      // ---- d gamma2, d beta2, d Wo, d bo
      sa_dln(H1, Y, LX, C, T, nact, slen, gp + of.g2, gp + of.be2, first);
      sa_dw<false>(O, G, nullptr, nullptr, LX, C, T, nact, slen, gp + of.Wo, gp + of.bo, first);
      __syncthreads();
      // ---- the attention backwards, both as a gather: d q -> O by the query's thread over its keys, d k -> H1 and d v -> Y
      // by the key's thread over the queries t' >= t of its history
      if (active) {
        for (int hd = 0; hd < nh; ++hd) {
          const int c0 = hd * dh;
          const float lse = st[hd], dl = st[nh + hd];
          for (int d = 0; d < dh; ++d) orow[c0 + d] = 0.f;
          for (int s = 0; s <= t; ++s) {
            const float* ks = K0 + s * LX + c0;
            const float a = expf(sa_dot(qr + c0, ks, dh) * scale - lse);
            const float dz = a * (sa_dot(t1 + c0, V0 + s * LX + c0, dh) - dl) * scale;
            for (int d = 0; d < dh; ++d) orow[c0 + d] = fmaf(dz, ks[d], orow[c0 + d]);
          }
          for (int d = 0; d < dh; ++d) h1[c0 + d] = 0.f, yr[c0 + d] = 0.f;
          for (int tq = t; tq < len; ++tq) {
            const int r = hs * T + tq;
            const float* qt = Q + r * LX + c0;
            const float* dot_ = T1 + r * LX + c0;
            const float a = expf(sa_dot(qt, kr + c0, dh) * scale - ST[r * LS + hd]);
            const float dz = a * (sa_dot(dot_, vr + c0, dh) - ST[r * LS + nh + hd]) * scale;
            for (int d = 0; d < dh; ++d) {
              h1[c0 + d] = fmaf(dz, qt[d], h1[c0 + d]);
              yr[c0 + d] = fmaf(a, dot_[d], yr[c0 + d]);
            }
          }
        }
      }
      __syncthreads();
      // ---- d u = d q . Wq^T + d k . Wk^T + d v . Wv^T -> Q; xhat1 -> T1; G += LN1 backward: G is d x_l
      if (active) {
        for (int c = 0; c < C; c += 4) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          sa_dot4(orow, p + of.Wq + c * C, C, C, acc);
          sa_dot4(h1, p + of.Wk + c * C, C, C, acc);
          sa_dot4(yr, p + of.Wv + c * C, C, C, acc);
          qr[c] = acc.x, qr[c + 1] = acc.y, qr[c + 2] = acc.z, qr[c + 3] = acc.w;
        }
        for (int c = 0; c < C; ++c) t1[c] = (xr[c] - mean1) * rstd1;
        sa_ln_bwd(qr, t1, p + of.g1, rstd1, C, gr);
      }
      __syncthreads();
      // ---- d Wq, d bq, d Wk, d bk, d Wv, d bv, d gamma1, d beta1
      sa_dw<true>(T1, O, p + of.g1, p + of.be1, LX, C, T, nact, slen, gp + of.Wq, gp + of.bq, first);
      sa_dw<true>(T1, H1, p + of.g1, p + of.be1, LX, C, T, nact, slen, gp + of.Wk, gp + of.bk, first);
      sa_dw<true>(T1, Y, p + of.g1, p + of.be1, LX, C, T, nact, slen, gp + of.Wv, gp + of.bv, first);
      sa_dln(Q, T1, LX, C, T, nact, slen, gp + of.g1, gp + of.be1, first);
    }
    __syncthreads();
    // ---- d hist = d x_0 (padding rows of G were never touched: zero); d pos[p] = sum over histories of d x_0[len - 1 - p]
    float* __restrict__ dst = dhist + base * T * C;
    for (int e = tid; e < rows * C; e += SA_THREADS) {
      const int r = e / C;
      dst[e] = G[r * LX + (e - r * C)];
    }
    for (int e = tid; e < Tmax * C; e += SA_THREADS) {
      const int pp = e / C, c = e - pp * C;
      float s = 0.f;
      for (int h = 0; h < nact; ++h)
        if (slen[h] > pp) s += G[(h * T + slen[h] - 1 - pp) * LX + c];
      sa_acc(part + e, first, s);
    }
  }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int clsr_sasrec_fwd(const float* hist, const int* seq_len, int len_stride, long Hn, int T, int Tmax, int C,
                               const float* params, int nblocks, int nheads, float* saved, float* out, int ldo, int rep,
                               void* stream) {
  CLSR_CHECK_ARG(hist && seq_len && params && out);
  CLSR_CHECK_ARG(Hn > 0 && rep >= 1 && ldo >= C && len_stride >= 1);
  CLSR_CHECK_SUPPORTED(clsr_sasrec_supported(T, Tmax, C, nblocks, nheads));
  CLSR_CHECK_SUPPORTED(Hn * T * (long)(rep > nblocks ? rep : nblocks) < (1L << 31) / SA_MAX_C);
  const int S = sa_slice(T, C, 0);
  const size_t shmem = (size_t)(S * sa_fwd_hist_floats(T, C) + sa_fixed_floats(S)) * sizeof(float);
  if (shmem > 64 * 1024)
    CLSR_HIP(hipFuncSetAttribute((const void*)sa_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  long grid = (Hn + S - 1) / S;
  if (grid > 2 * SA_MAX_PARTS) grid = 2 * SA_MAX_PARTS;
  hipLaunchKernelGGL(sa_fwd_kernel, dim3((unsigned)grid), dim3(SA_THREADS), shmem, (hipStream_t)stream, hist, seq_len,
                     len_stride, Hn, T, C, params, Tmax, nblocks, nheads, saved, out, ldo, rep, S);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_sasrec_bwd(const float* dout, const float* saved, const int* seq_len, int len_stride, long Hn, int T,
                               int Tmax, int C, const float* params, int nblocks, int nheads, float* dhist,
                               float* partial, void* stream) {
  CLSR_CHECK_ARG(dout && saved && seq_len && params && dhist && partial);
  CLSR_CHECK_ARG(Hn > 0 && len_stride >= 1);
  CLSR_CHECK_SUPPORTED(clsr_sasrec_supported(T, Tmax, C, nblocks, nheads));
  CLSR_CHECK_SUPPORTED(Hn * T * (long)nblocks < (1L << 31) / SA_MAX_C);
  const int S = sa_slice(T, C, 1);
  const size_t shmem = (size_t)(S * sa_bwd_hist_floats(T, C) + sa_fixed_floats(S)) * sizeof(float);
  if (shmem > 64 * 1024)
    CLSR_HIP(hipFuncSetAttribute((const void*)sa_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  const int parts = clsr_sasrec_parts(Hn, T, Tmax, C, nblocks);
  hipLaunchKernelGGL(sa_bwd_kernel, dim3((unsigned)parts), dim3(SA_THREADS), shmem, (hipStream_t)stream, dout, saved,
                     seq_len, len_stride, Hn, T, C, params, Tmax, nblocks, nheads, dhist, partial, S);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ================================================================================================ tiled kernels
// The same encoder for histories whose backward state LDS does not hold (and for any it does): a workgroup owns ONE history
// at a time and walks its steps in tiles of TE = min(tile, T) rows; thread r of the first TE owns row t0 + r of the tile.
// k and v of the WHOLE history stay in LDS (two rows per step), every other row exists for one tile only:
//   forward   LDS: 2 T (C + 1) + 3 TE (C + 1) words (k, v | x, q, o).  One sweep per block, tiles ascending: a tile's keys
//             0 .. t are in place when its queries attend (causal).  A block's output rows go to the next block's rows of
//             ``saved`` (training) or to the workgroup's T C floats of the workspace (scoring) and come back tile by tile.
//   backward  LDS: 2 T (C + 1) + 7 TE (C + 1) + TE (C / 2 + 1) words (k, v | x, xhat2, q, o, the gradient, two scratch rows,
//             log-sum-exp and sum a da per head).  The gradient w.r.t. a block's output lives in the history's rows of
//             dhist between tiles.  Two sweeps per block:
//             the QUERY sweep recomputes a tile (k, v into the resident rows), walks it back to d q, adds d W2 .. d Wq,
//             and parks per row q | d o | d q Wq^T | log-sum-exp, sum a da in the workgroup's rows of the workspace
//             (3 C + C / 2 floats a row);
//             the KEY sweep takes a tile of keys, streams the parked rows of the query tiles i >= j back through the
//             staging rows (tiles ascending, rows ascending), sums d k and d v into the key tile's own rows, finishes d u,
//             the first layer norm's backward and d Wk, d Wv, d gamma1, d beta1.
// Dense gradients: the workgroup zeroes its row of partial sums once, then one owner thread per element adds a tile's rows
// (ascending) to it, tiles ascending, histories ascending.  No atomics: two runs are bit-identical.
#define SA_TILE_MAX 64

static inline int sa_tile_rows(int T, int tile) { return tile < T ? tile : T; }
static inline long sa_tiled_lds_floats(int T, int C, int tile, int training) {
  return 2L * T * (C + 1) + (long)sa_tile_rows(T, tile) * (training ? 7L * (C + 1) + C / 2 + 1 : 3L * (C + 1));
}
// floats of a parked row: q [C] | d o [C] | d q Wq^T [C] | log-sum-exp [nh] | sum a da [nh] (2 nh <= C / 2)
__host__ __device__ static inline int sa_park_floats(int C) { return 3 * C + C / 2; }

extern "C" long clsr_sasrec_tiled_lds_bytes(int T, int C, int tile, int training) {
  if (T <= 0 || C <= 0 || tile <= 0) return 0;
  return 4L * sa_tiled_lds_floats(T, C, tile, training);
}

extern "C" int clsr_sasrec_tiled_supported(int T, int Tmax, int C, int nblocks, int nheads, int tile) {
  if (!sa_dims_ok(T, C) || Tmax < T || Tmax > SA_MAX_T) return 0;
  if (nblocks < 1 || nblocks > SA_MAX_BLOCKS || nheads < 1 || C % nheads || (C / nheads) % 4) return 0;
  if (tile < 1 || tile > SA_TILE_MAX) return 0;
  return clsr_sasrec_tiled_lds_bytes(T, C, tile, 1) <= clsr_sasrec_lds_budget_bytes();
}

// the tile the host passes: the largest the budget holds, at most SA_TILE_MAX (0: none fits)
extern "C" int clsr_sasrec_tiled_default_tile(int T, int C) {
  if (!sa_dims_ok(T, C)) return 0;
  for (int tile = SA_TILE_MAX; tile >= 1; --tile)
    if (clsr_sasrec_tiled_lds_bytes(T, C, tile, 1) <= clsr_sasrec_lds_budget_bytes()) return tile;
  return 0;
}

// workgroups of both launches = rows of partial sums = sets of parked rows
extern "C" int clsr_sasrec_tiled_parts(long Hn, int T, int Tmax, int C, int nblocks) {
  if (Hn <= 0 || !clsr_sasrec_tiled_supported(T, Tmax, C, nblocks, 1, 1)) return 0;
  long parts = Hn < SA_MAX_PARTS ? Hn : SA_MAX_PARTS;
  const long cap = SA_WS_FLOATS / (clsr_sasrec_param_floats(Tmax, C, nblocks) + (long)T * sa_park_floats(C));
  if (parts > cap) parts = cap;
  return parts < 1 ? 1 : (int)parts;
}

// training: [parts][param floats] partial sums, then [parts][T][3 C + C / 2] parked rows; scoring: [parts][T][C] rows of x
extern "C" long clsr_sasrec_tiled_workspace_floats(long Hn, int T, int Tmax, int C, int nblocks, int tile, int training) {
  if (!clsr_sasrec_tiled_supported(T, Tmax, C, nblocks, 1, tile)) return 0;
  const long parts = clsr_sasrec_tiled_parts(Hn, T, Tmax, C, nblocks);
  return parts * (training ? clsr_sasrec_param_floats(Tmax, C, nblocks) + (long)T * sa_park_floats(C) : (long)T * C);
}

__device__ __forceinline__ int sa_len(const int* __restrict__ seq_len, int len_stride, long h, int T) {
  const int n = seq_len[h * len_stride];
  return n < 0 ? 0 : (n > T ? T : n);
}

// ------------------------------------------------------------------------------------------------ tiled forward
// xs: the workgroup's [T][C] rows of x between blocks (scoring; training keeps them in saved)
__global__ void __launch_bounds__(SA_THREADS) sa_tiled_fwd_kernel(const float* __restrict__ hist,
                                                                  const int* __restrict__ seq_len, int len_stride, long Hn,
                                                                  int T, int C, const float* __restrict__ params, int Tmax,
                                                                  int nb, int nh, float* saved, float* __restrict__ out,
                                                                  int ldo, int rep, int TE, float* ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, LX = C + 1, dh = C / nh;
  float* K = lds;
  float* V = K + T * LX;
  float* X = V + T * LX;
  float* Q = X + TE * LX;
  float* O = Q + TE * LX;
  const SaOff of = sa_offsets(C);
  const long PB = sa_block_floats(C), TC = (long)T * C;
  const float* __restrict__ pos = params;
  const float* __restrict__ blocks = params + (long)Tmax * C;
  const float* __restrict__ fin = blocks + nb * PB;
  const float scale = 1.0f / sqrtf((float)dh);
  float* xs = saved ? nullptr : ws + (long)blockIdx.x * TC;
  for (long h = blockIdx.x; h < Hn; h += gridDim.x) {
    const int len = sa_len(seq_len, len_stride, h, T);
    const float* __restrict__ src = hist + h * TC;
    if (saved)      // the rows of padding of every block's input
      for (int l = 0; l < nb; ++l)
        for (long e = (long)len * C + tid; e < TC; e += SA_THREADS) saved[((long)l * Hn + h) * TC + e] = 0.f;
    if (len == 0) {
      for (int c = tid; c < C; c += SA_THREADS) {
        if (saved) saved[(long)nb * Hn * TC + h * C + c] = 0.f;
        for (int g = 0; g < rep; ++g) out[(h * rep + g) * ldo + c] = 0.f;
      }
      continue;
    }
    const int ntv = (len + TE - 1) / TE;
    for (int l = 0; l < nb; ++l) {
      const float* __restrict__ p = blocks + l * PB;
      const float* xin = saved ? saved + ((long)l * Hn + h) * TC : xs;
      float* xout = l + 1 < nb ? (saved ? saved + ((long)(l + 1) * Hn + h) * TC : xs) : nullptr;
      for (int j = 0; j < ntv; ++j) {
        const int t0 = j * TE, nr = min(TE, len - t0);
        __syncthreads();
        for (int e = tid; e < nr * C; e += SA_THREADS) {
          const int r = e / C, c = e - r * C, tt = t0 + r;
          float v;
          if (l == 0) {
            v = src[tt * C + c] + pos[(len - 1 - tt) * C + c];
            if (saved) saved[h * TC + tt * C + c] = v;
          } else {
            v = xin[tt * C + c];
          }
          X[r * LX + c] = v;
        }
        __syncthreads();
        const bool active = tid < nr;
        const int row = active ? tid : 0, t = t0 + row;
        float* xr = X + row * LX;
        float* qr = Q + row * LX;
        float* orow = O + row * LX;
        if (active) {
          float mean, rstd;
          sa_stats(xr, C, mean, rstd);
          sa_qkv(xr, mean, rstd, orow, p, of, C, qr, K + t * LX, V + t * LX);
        }
        __syncthreads();
        if (active) {
          sa_attend(qr, K, V, LX, t, nh, dh, scale, orow, nullptr);
          for (int o = 0; o < C; o += 4) {
            f32x4 acc = ld4(p + of.bo + o);
            sa_axpy4(orow, p + of.Wo + o, C, C, acc);
            xr[o] += acc.x, xr[o + 1] += acc.y, xr[o + 2] += acc.z, xr[o + 3] += acc.w;
          }
          float mean, rstd;
          sa_stats(xr, C, mean, rstd);
          for (int c = 0; c < C; ++c) orow[c] = (xr[c] - mean) * rstd;
          for (int o = 0; o < C; o += 4) {
            f32x4 acc = ld4(p + of.b1 + o);
            sa_axpy4_ln(orow, p + of.g2, p + of.be2, p + of.W1 + o, C, C, acc);
            qr[o] = sa_relu(acc.x), qr[o + 1] = sa_relu(acc.y), qr[o + 2] = sa_relu(acc.z), qr[o + 3] = sa_relu(acc.w);
          }
          for (int o = 0; o < C; o += 4) {
            f32x4 acc = ld4(p + of.b2 + o);
            sa_axpy4(qr, p + of.W2 + o, C, C, acc);
            xr[o] += acc.x, xr[o + 1] += acc.y, xr[o + 2] += acc.z, xr[o + 3] += acc.w;
          }
          // ---- s = LNf(x_L[len - 1]), once per row of the history group
          if (l == nb - 1 && t == len - 1) {
            float mf, rf;
            sa_stats(xr, C, mf, rf);
            if (saved)
              for (int c = 0; c < C; ++c) saved[(long)nb * Hn * TC + h * C + c] = xr[c];
            for (int c = 0; c < C; ++c) {
              const float v = fmaf(fin[c], (xr[c] - mf) * rf, fin[C + c]);
              for (int g = 0; g < rep; ++g) out[(h * rep + g) * ldo + c] = v;
            }
          }
        }
        if (xout) {
          __syncthreads();
          for (int e = tid; e < nr * C; e += SA_THREADS) {
            const int r = e / C, c = e - r * C;
            xout[(t0 + r) * C + c] = X[r * LX + c];
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ tiled backward
// gp[e] += sum over the tile's rows r < nr of A(r, e / C) * Bm[r][e % C] (one owner thread per element, rows ascending; LN as
// in sa_dw); then the column sums of Bm are added to gb (NULL: none)
template <bool LN>
__device__ __forceinline__ void sa_dw_add(const float* Am, const float* Bm, const float* __restrict__ g,
                                          const float* __restrict__ b, int LX, int C, int nr, float* gp, float* gb) {
  for (int e = threadIdx.x; e < C * C; e += SA_THREADS) {
    const int i = e / C, o = e - i * C;
    const float gi = LN ? g[i] : 1.f, bi = LN ? b[i] : 0.f;
    float s = 0.f;
    for (int r = 0; r < nr; ++r) s = fmaf(LN ? fmaf(gi, Am[r * LX + i], bi) : Am[r * LX + i], Bm[r * LX + o], s);
    gp[e] += s;
  }
  if (gb)
    for (int o = threadIdx.x; o < C; o += SA_THREADS) {
      float s = 0.f;
      for (int r = 0; r < nr; ++r) s += Bm[r * LX + o];
      gb[o] += s;
    }
}

// d gamma[c] += sum_r Dm[r][c] * Xh[r][c], d beta[c] += sum_r Dm[r][c] over the tile's rows
__device__ __forceinline__ void sa_dln_add(const float* Dm, const float* Xh, int LX, int C, int nr, float* gg, float* gb) {
  for (int c = threadIdx.x; c < C; c += SA_THREADS) {
    float sg = 0.f, sb = 0.f;
    for (int r = 0; r < nr; ++r) {
      const float d = Dm[r * LX + c];
      sg = fmaf(d, Xh[r * LX + c], sg);
      sb += d;
    }
    gg[c] += sg;
    gb[c] += sb;
  }
}

__global__ void __launch_bounds__(SA_THREADS) sa_tiled_bwd_kernel(const float* __restrict__ dout,
                                                                  const float* __restrict__ saved,
                                                                  const int* __restrict__ seq_len, int len_stride, long Hn,
                                                                  int T, int C, const float* __restrict__ params, int Tmax,
                                                                  int nb, int nh, float* dhist, float* partial, int TE,
                                                                  float* parked) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, LX = C + 1, LS = C / 2 + 1, dh = C / nh, WR = sa_park_floats(C);
  const int BUF = TE * LX;
  float* K = lds;             // the whole history
  float* V = K + T * LX;
  float* X = V + T * LX;      // the tile: the block's input x_l
  float* Y = X + BUF;         // xhat2; key sweep: d v
  float* Q = Y + BUF;         // q; key sweep: the staged q, then d u
  float* O = Q + BUF;         // o, then d q
  float* G = O + BUF;         // gradient w.r.t. the block's output, then its input
  float* T1 = G + BUF;        // d h1, then d o, then xhat1; key sweep: the staged d o, then xhat1
  float* H1 = T1 + BUF;       // h1, then d w, then d q Wq^T; key sweep: d k
  float* ST = H1 + BUF;       // per row: log-sum-exp [nh] | sum a da [nh]
  const SaOff of = sa_offsets(C);
  const long PB = sa_block_floats(C), TC = (long)T * C;
  const long P = (long)Tmax * C + nb * PB + 2 * C;
  const float* __restrict__ blocks = params + (long)Tmax * C;
  const float* __restrict__ fin = blocks + nb * PB;
  const float scale = 1.0f / sqrtf((float)dh);
  float* part = partial + (long)blockIdx.x * P;
  float* part_blocks = part + (long)Tmax * C;
  float* part_fin = part_blocks + nb * PB;
  float* park = parked + (long)blockIdx.x * T * WR;
  const float* __restrict__ xlast = saved + (long)nb * Hn * TC;
  for (long e = tid; e < P; e += SA_THREADS) part[e] = 0.f;
  for (long h = blockIdx.x; h < Hn; h += gridDim.x) {
    const int len = sa_len(seq_len, len_stride, h, T);
    float* dx = dhist + h * TC;     // the history's gradient rows between tiles; d hist at the end
    __syncthreads();
    for (long e = tid; e < TC; e += SA_THREADS) dx[e] = 0.f;
    if (len == 0) continue;
    // ---- the final layer norm (row len - 1 only): xhatf -> T1, d s -> H1, its backward -> G, in row 0 of the tile
    if (tid == 0) {
      const float* __restrict__ xl = xlast + h * C;
      const float* __restrict__ ds = dout + h * C;
      for (int c = 0; c < C; ++c) T1[c] = xl[c];
      float mean, rstd;
      sa_stats(T1, C, mean, rstd);
      for (int c = 0; c < C; ++c) T1[c] = (T1[c] - mean) * rstd, H1[c] = ds[c], G[c] = 0.f;
      sa_ln_bwd(H1, T1, fin, rstd, C, G);
    }
    __syncthreads();
    for (int c = tid; c < C; c += SA_THREADS) {
      part_fin[c] += H1[c] * T1[c];
      part_fin[C + c] += H1[c];
      dx[(long)(len - 1) * C + c] = G[c];
    }
    const int ntv = (len + TE - 1) / TE;
    for (int l = nb - 1; l >= 0; --l) {
      const float* __restrict__ p = blocks + l * PB;
      float* gp = part_blocks + l * PB;
      const float* __restrict__ xsrc = saved + ((long)l * Hn + h) * TC;
      // ================================================================ the query sweep
      for (int j = 0; j < ntv; ++j) {
        const int t0 = j * TE, nr = min(TE, len - t0);
        __syncthreads();
        for (int e = tid; e < nr * C; e += SA_THREADS) {
          const int r = e / C, c = e - r * C;
          X[r * LX + c] = xsrc[(t0 + r) * C + c];
          G[r * LX + c] = dx[(t0 + r) * C + c];
        }
        __syncthreads();
        const bool active = tid < nr;
        const int row = active ? tid : 0, t = t0 + row;
        float* xr = X + row * LX;
        float* yr = Y + row * LX;
        float* qr = Q + row * LX;
        float* kr = K + t * LX;
        float* vr = V + t * LX;
        float* orow = O + row * LX;
        float* gr = G + row * LX;
        float* t1 = T1 + row * LX;
        float* h1 = H1 + row * LX;
        float* st = ST + row * LS;
        // ---- the block again: q, k, v
        float mean1 = 0.f, rstd1 = 0.f, rstd2 = 0.f;
        if (active) {
          sa_stats(xr, C, mean1, rstd1);
          sa_qkv(xr, mean1, rstd1, orow, p, of, C, qr, kr, vr);
        }
        __syncthreads();
        // ---- o and the log-sum-exp, xhat2 -> Y, h1 -> H1, then d h1 = gate (G . W2^T) -> T1
        if (active) {
          sa_attend(qr, K, V, LX, t, nh, dh, scale, orow, st);
          for (int o = 0; o < C; o += 4) {
            f32x4 acc = ld4(p + of.bo + o);
            sa_axpy4(orow, p + of.Wo + o, C, C, acc);
            yr[o] = xr[o] + acc.x, yr[o + 1] = xr[o + 1] + acc.y, yr[o + 2] = xr[o + 2] + acc.z, yr[o + 3] = xr[o + 3] + acc.w;
          }
          float mean2;
          sa_stats(yr, C, mean2, rstd2);
          for (int c = 0; c < C; ++c) yr[c] = (yr[c] - mean2) * rstd2;
          for (int o = 0; o < C; o += 4) {
            f32x4 acc = ld4(p + of.b1 + o);
            sa_axpy4_ln(yr, p + of.g2, p + of.be2, p + of.W1 + o, C, C, acc);
            h1[o] = sa_relu(acc.x), h1[o + 1] = sa_relu(acc.y), h1[o + 2] = sa_relu(acc.z), h1[o + 3] = sa_relu(acc.w);
          }
          for (int jj = 0; jj < C; jj += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            sa_dot4(gr, p + of.W2 + jj * C, C, C, acc);
            t1[jj] = h1[jj] > 0.f ? acc.x : 0.f, t1[jj + 1] = h1[jj + 1] > 0.f ? acc.y : 0.f;
            t1[jj + 2] = h1[jj + 2] > 0.f ? acc.z : 0.f, t1[jj + 3] = h1[jj + 3] > 0.f ? acc.w : 0.f;
          }
        }
        __syncthreads();
        // ---- d W2, d b2, d W1, d b1
        sa_dw_add<false>(H1, G, nullptr, nullptr, LX, C, nr, gp + of.W2, gp + of.b2);
        sa_dw_add<true>(Y, T1, p + of.g2, p + of.be2, LX, C, nr, gp + of.W1, gp + of.b1);
        __syncthreads();
        // ---- d w = d h1 . W1^T -> H1; G += LN2 backward: G is d y; d o = d y . Wo^T -> T1; sum a da per head = d o . o
        if (active) {
          for (int c = 0; c < C; c += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            sa_dot4(t1, p + of.W1 + c * C, C, C, acc);
            h1[c] = acc.x, h1[c + 1] = acc.y, h1[c + 2] = acc.z, h1[c + 3] = acc.w;
          }
          sa_ln_bwd(h1, yr, p + of.g2, rstd2, C, gr);
          for (int c = 0; c < C; c += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            sa_dot4(gr, p + of.Wo + c * C, C, C, acc);
            t1[c] = acc.x, t1[c + 1] = acc.y, t1[c + 2] = acc.z, t1[c + 3] = acc.w;
          }
          for (int hd = 0; hd < nh; ++hd) st[nh + hd] = sa_dot(t1 + hd * dh, orow + hd * dh, dh);
        }
        __syncthreads();
        // ---- d gamma2, d beta2, d Wo, d bo
        sa_dln_add(H1, Y, LX, C, nr, gp + of.g2, gp + of.be2);
        sa_dw_add<false>(O, G, nullptr, nullptr, LX, C, nr, gp + of.Wo, gp + of.bo);
        __syncthreads();
        // ---- d q -> O by the query's thread over its keys; the row is parked for the key sweep; d q Wq^T -> H1 and parked;
        // xhat1 -> T1
        if (active) {
          float* pk = park + (long)t * WR;
          for (int hd = 0; hd < nh; ++hd) {
            const int c0 = hd * dh;
            const float lse = st[hd], dl = st[nh + hd];
            for (int d = 0; d < dh; ++d) orow[c0 + d] = 0.f;
            for (int s = 0; s <= t; ++s) {
              const float* ks = K + s * LX + c0;
              const float a = expf(sa_dot(qr + c0, ks, dh) * scale - lse);
              const float dz = a * (sa_dot(t1 + c0, V + s * LX + c0, dh) - dl) * scale;
              for (int d = 0; d < dh; ++d) orow[c0 + d] = fmaf(dz, ks[d], orow[c0 + d]);
            }
            pk[3 * C + hd] = lse, pk[3 * C + nh + hd] = dl;
          }
          for (int c = 0; c < C; ++c) pk[c] = qr[c], pk[C + c] = t1[c];
          for (int c = 0; c < C; c += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            sa_dot4(orow, p + of.Wq + c * C, C, C, acc);
            pk[2 * C + c] = acc.x, pk[2 * C + c + 1] = acc.y, pk[2 * C + c + 2] = acc.z, pk[2 * C + c + 3] = acc.w;
          }
          for (int c = 0; c < C; ++c) t1[c] = (xr[c] - mean1) * rstd1;
        }
        __syncthreads();
        // ---- d Wq, d bq; the gradient rows (d y) go back
        sa_dw_add<true>(T1, O, p + of.g1, p + of.be1, LX, C, nr, gp + of.Wq, gp + of.bq);
        for (int e = tid; e < nr * C; e += SA_THREADS) {
          const int r = e / C, c = e - r * C;
          dx[(t0 + r) * C + c] = G[r * LX + c];
        }
      }
      // ================================================================ the key sweep
      for (int j = 0; j < ntv; ++j) {
        const int t0 = j * TE, nr = min(TE, len - t0);
        __syncthreads();
        for (int e = tid; e < nr * C; e += SA_THREADS) {
          const int r = e / C, c = e - r * C;
          X[r * LX + c] = xsrc[(t0 + r) * C + c];
          G[r * LX + c] = dx[(t0 + r) * C + c];
        }
        const bool active = tid < nr;
        const int row = active ? tid : 0, t = t0 + row;
        float* xr = X + row * LX;
        float* yr = Y + row * LX;
        float* qr = Q + row * LX;
        const float* kr = K + t * LX;
        const float* vr = V + t * LX;
        float* gr = G + row * LX;
        float* t1 = T1 + row * LX;
        float* h1 = H1 + row * LX;
        if (active)
          for (int c = 0; c < C; ++c) h1[c] = 0.f, yr[c] = 0.f;
        // ---- d k -> H1 and d v -> Y by the key's thread over the queries t' >= t, a staged tile of parked rows at a time
        for (int i = j; i < ntv; ++i) {
          const int q0 = i * TE, nq = min(TE, len - q0);
          __syncthreads();
          for (int e = tid; e < nq * C; e += SA_THREADS) {
            const int r = e / C, c = e - r * C;
            const float* pk = park + (long)(q0 + r) * WR;
            Q[r * LX + c] = pk[c];
            T1[r * LX + c] = pk[C + c];
          }
          for (int e = tid; e < nq * 2 * nh; e += SA_THREADS) {
            const int r = e / (2 * nh), k2 = e - r * 2 * nh;
            ST[r * LS + k2] = park[(long)(q0 + r) * WR + 3 * C + k2];
          }
          __syncthreads();
          if (active)
            for (int hd = 0; hd < nh; ++hd) {
              const int c0 = hd * dh;
              for (int tq = max(t, q0); tq < q0 + nq; ++tq) {
                const int r = tq - q0;
                const float* qt = Q + r * LX + c0;
                const float* dot_ = T1 + r * LX + c0;
                const float a = expf(sa_dot(qt, kr + c0, dh) * scale - ST[r * LS + hd]);
                const float dz = a * (sa_dot(dot_, vr + c0, dh) - ST[r * LS + nh + hd]) * scale;
                for (int d = 0; d < dh; ++d) {
                  h1[c0 + d] = fmaf(dz, qt[d], h1[c0 + d]);
                  yr[c0 + d] = fmaf(a, dot_[d], yr[c0 + d]);
                }
              }
            }
        }
        __syncthreads();
        // ---- d u = d q . Wq^T (parked) + d k . Wk^T + d v . Wv^T -> Q; xhat1 -> T1; G += LN1 backward: G is d x_l
        if (active) {
          float mean1, rstd1;
          sa_stats(xr, C, mean1, rstd1);
          const float* pk = park + (long)t * WR + 2 * C;
          for (int c = 0; c < C; c += 4) {
            f32x4 acc = {pk[c], pk[c + 1], pk[c + 2], pk[c + 3]};
            sa_dot4(h1, p + of.Wk + c * C, C, C, acc);
            sa_dot4(yr, p + of.Wv + c * C, C, C, acc);
            qr[c] = acc.x, qr[c + 1] = acc.y, qr[c + 2] = acc.z, qr[c + 3] = acc.w;
          }
          for (int c = 0; c < C; ++c) t1[c] = (xr[c] - mean1) * rstd1;
          sa_ln_bwd(qr, t1, p + of.g1, rstd1, C, gr);
        }
        __syncthreads();
        // ---- d Wk, d bk, d Wv, d bv, d gamma1, d beta1; the gradient rows (d x_l) go back
        sa_dw_add<true>(T1, H1, p + of.g1, p + of.be1, LX, C, nr, gp + of.Wk, gp + of.bk);
        sa_dw_add<true>(T1, Y, p + of.g1, p + of.be1, LX, C, nr, gp + of.Wv, gp + of.bv);
        sa_dln_add(Q, T1, LX, C, nr, gp + of.g1, gp + of.be1);
        for (int e = tid; e < nr * C; e += SA_THREADS) {
          const int r = e / C, c = e - r * C;
          dx[(t0 + r) * C + c] = G[r * LX + c];
        }
      }
    }
    __syncthreads();
    // ---- dx is d hist (padding rows zero); d pos[p] += d x_0[len - 1 - p]
    for (int e = tid; e < len * C; e += SA_THREADS) {
      const int pp = e / C, c = e - pp * C;
      part[e] += dx[(long)(len - 1 - pp) * C + c];
    }
  }
}

extern "C" int clsr_sasrec_tiled_fwd(const float* hist, const int* seq_len, int len_stride, long Hn, int T, int Tmax, int C,
                                     const float* params, int nblocks, int nheads, float* saved, float* out, int ldo,
                                     int rep, int tile, float* workspace, void* stream) {
  CLSR_CHECK_ARG(hist && seq_len && params && out && (saved || workspace));
  CLSR_CHECK_ARG(Hn > 0 && rep >= 1 && ldo >= C && len_stride >= 1);
  CLSR_CHECK_SUPPORTED(clsr_sasrec_tiled_supported(T, Tmax, C, nblocks, nheads, tile));
  CLSR_CHECK_SUPPORTED(Hn * T * (long)(rep > nblocks ? rep : nblocks) < (1L << 31) / SA_MAX_C);
  const size_t shmem = (size_t)sa_tiled_lds_floats(T, C, tile, 0) * sizeof(float);
  if (shmem > 64 * 1024)
    CLSR_HIP(hipFuncSetAttribute((const void*)sa_tiled_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  const int parts = clsr_sasrec_tiled_parts(Hn, T, Tmax, C, nblocks);
  hipLaunchKernelGGL(sa_tiled_fwd_kernel, dim3((unsigned)parts), dim3(SA_THREADS), shmem, (hipStream_t)stream, hist, seq_len,
                     len_stride, Hn, T, C, params, Tmax, nblocks, nheads, saved, out, ldo, rep, sa_tile_rows(T, tile),
                     workspace);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_sasrec_tiled_bwd(const float* dout, const float* saved, const int* seq_len, int len_stride, long Hn,
                                     int T, int Tmax, int C, const float* params, int nblocks, int nheads, float* dhist,
                                     int tile, float* workspace, void* stream) {
  CLSR_CHECK_ARG(dout && saved && seq_len && params && dhist && workspace);
  CLSR_CHECK_ARG(Hn > 0 && len_stride >= 1);
  CLSR_CHECK_SUPPORTED(clsr_sasrec_tiled_supported(T, Tmax, C, nblocks, nheads, tile));
  CLSR_CHECK_SUPPORTED(Hn * T * (long)nblocks < (1L << 31) / SA_MAX_C);
  const size_t shmem = (size_t)sa_tiled_lds_floats(T, C, tile, 1) * sizeof(float);
  if (shmem > 64 * 1024)
    CLSR_HIP(hipFuncSetAttribute((const void*)sa_tiled_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  const int parts = clsr_sasrec_tiled_parts(Hn, T, Tmax, C, nblocks);
  float* parked = workspace + (long)parts * clsr_sasrec_param_floats(Tmax, C, nblocks);
  hipLaunchKernelGGL(sa_tiled_bwd_kernel, dim3((unsigned)parts), dim3(SA_THREADS), shmem, (hipStream_t)stream, dout, saved,
                     seq_len, len_stride, Hn, T, C, params, Tmax, nblocks, nheads, dhist, workspace, sa_tile_rows(T, tile),
                     parked);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}
