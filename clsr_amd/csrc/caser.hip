// Caser (models/sequential/caser.py): the graph between the history gather and model_output, per embedding table
// (item | cate), over the history lookup X [Hn, T, Dx] (columns col0 .. col0 + Dx of the [Hn, T, D] history buffer):
//
//   vertical    out_v[b, f]    = relu(bv[f] + sum_{t < T} sum_{d < Dx} X[b, t, d] * Wv[d, t, f])             f < n_v
//   horizontal  c_h[b, t, f]   = bh_h[f] + sum_{j < h} sum_{d < Dx} X[b, t + j, d] * Wh_h[j, d, f]            t <= T - h
//               out_h[b, h, f] = relu(max_t c_h[b, t, f])                                          h = 1 .. L, f < n_h
//
// NO mask: the padded steps (embedding row 0) take part in every product and in the max, as in the reference.
//
// Parameter block of one table (floats; the order the reference creates the variables in, each tensor contiguous):
//   Wv [Dx][T][n_v] | bv [n_v] | Wh_1 [1][Dx][n_h] | bh_1 [n_h] | ... | Wh_L [L][Dx][n_h] | bh_L [n_h]
// n_v and n_h are multiples of 4, so every tensor starts 16-byte aligned and the block has no padding; the gradient
// block has the same layout.  Pooled block of one table: [out_v (n_v) | out_h(1) (n_h) | ... | out_h(L) (n_h)].
//
// Arithmetic: plain fp32 FMA chains (the fp32-input MFMAs of this chip run at the vector FMA rate; the products are
// small).  The accumulation order per (b, t, f) is fixed -- bias, then j ascending, d ascending -- and the same
// instruction sequence serves every position, so windows with identical inputs give bit-identical values: the first
// maximum and the set of positions TIED with it are deterministic.  The gradient of a pool is split evenly among the
// tied positions, as tf.reduce_max's gradient does (ties are systematic here: every window that lies wholly in the
// padded region, every repeated item under a width-1 filter).  The split leaves the weight and table gradients of
// identical windows unchanged, but the per-position rows of d hist are the IndexedSlices the clip norm is taken over.
// ties [Hn][L][n_h][1 + ceil(T / 32)] (int32): number of tied positions | bit t of the mask: c_h[t] equals the maximum
// (bits below the first maximum are stale and never read).
// No atomics anywhere: every output element has one owner thread; the weight gradients are per-slice partial sums
// reduced in ascending slice order.
#include "common.h"

#define CZ_TC 8            // positions per register tile
#define CZ_CH 64           // positions per LDS chunk (at most; a multiple of CZ_TC)
#define CZ_LDS_FLOATS 16384
#define CZ_MAX_FILTERS 1024
#define CZ_WS_FLOATS (1L << 26)

// floats of Wh_h | bh_h
__host__ __device__ static inline long cz_hblock(int Dx, int h, int nh) { return (long)h * Dx * nh + nh; }
static inline long cz_hbase(int T, int Dx, int nv) { return (long)Dx * T * nv + nv; }
static inline long cz_block(int T, int Dx, int L, int nv, int nh) {
  return cz_hbase(T, Dx, nv) + (long)Dx * nh * ((long)L * (L + 1) / 2) + (long)L * nh;
}
__device__ __forceinline__ long cz_hoff(int T, int Dx, int nv, int nh, int h) {   // offset of Wh_h in the block
  return (long)Dx * T * nv + nv + (long)Dx * nh * ((long)h * (h - 1) / 2) + (long)(h - 1) * nh;
}

// positions per LDS chunk for this shape (0: the chunk plus its overlap of L - 1 positions does not fit)
static int cz_chunk(int T, int Di, int Dc, int L) {
  const int Dm = Di > Dc ? Di : Dc;
  const int rows = CZ_LDS_FLOATS / Dm;
  int ch = (rows - (L - 1)) / CZ_TC * CZ_TC;
  if (ch > CZ_CH) ch = CZ_CH;
  const int tpad = (T + CZ_TC - 1) / CZ_TC * CZ_TC;
  if (ch > tpad) ch = tpad;
  return ch < CZ_TC ? 0 : ch;
}

extern "C" int clsr_caser_supported(int T, int Di, int Dc, int L, int n_v, int n_h) {
  if (T <= 0 || T > 256 || Di <= 0 || Dc <= 0 || Di % 4 || Dc % 4 || Di + Dc > 256) return 0;
  if (L < 1 || L > T) return 0;
  if (n_v <= 0 || n_h <= 0 || n_v % 4 || n_h % 4 || n_v > CZ_MAX_FILTERS || n_h > CZ_MAX_FILTERS) return 0;
  if (cz_chunk(T, Di, Dc, L) == 0) return 0;
  // backward: the gated gradients, first maxima and tie counts of one history sit in LDS
  if ((long)n_v + 3L * L * n_h > CZ_LDS_FLOATS) return 0;
  return 1;
}

extern "C" int clsr_caser_max_filters(void) { return CZ_MAX_FILTERS; }

extern "C" long clsr_caser_param_floats(int T, int Dx, int L, int n_v, int n_h) { return cz_block(T, Dx, L, n_v, n_h); }

// ------------------------------------------------------------------------------------------------ forward
// One workgroup per (history, table).  The [T, Dx] tile goes through LDS in chunks of CH positions plus the L - 1 that
// the widest window of the chunk's last position reaches; a thread owns whole output columns (a vertical filter or one
// (h, f) pair), so its running sum / running maximum lives in the output arrays between chunks.
__global__ void __launch_bounds__(256) caser_fwd_kernel(const float* __restrict__ hist, int ldh, int T, int Di, int Dc,
                                                       const float* __restrict__ Wi, const float* __restrict__ Wc,
                                                       int L, int nv, int nh, int CH, float* __restrict__ pooled,
                                                       int ldp, int* __restrict__ amax_i, int* __restrict__ amax_c,
                                                       int* __restrict__ ties_i, int* __restrict__ ties_c) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const int tab = blockIdx.y, tid = threadIdx.x;
  const long b = blockIdx.x;
  const int Dx = tab ? Dc : Di, col0 = tab ? Di : 0;
  const float* __restrict__ W = tab ? Wc : Wi;
  int* __restrict__ amax = (tab ? amax_c : amax_i) + b * L * nh;
  const int TS = 1 + ((T + 31) >> 5);
  int* __restrict__ ties = (tab ? ties_c : ties_i) + b * L * nh * TS;
  const int PW = nv + L * nh;
  float* __restrict__ po = pooled + b * ldp + (long)tab * PW;
  const int rows = CH + L - 1, D4 = Dx >> 2;
  const float* __restrict__ xg = hist + b * T * ldh + col0;
  for (int t0 = 0; t0 < T; t0 += CH) {
    const bool first = t0 == 0, last = t0 + CH >= T;
    __syncthreads();
    for (int e = tid; e < rows * D4; e += 256) {
      const int r = e / D4, d = (e - r * D4) * 4, t = t0 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (t < T) v = *reinterpret_cast<const f32x4*>(xg + (long)t * ldh + d);
      *reinterpret_cast<f32x4*>(xs + r * Dx + d) = v;
    }
    __syncthreads();
    const int tend = min(t0 + CH, T);
    for (int c = tid; c < PW; c += 256) {
      if (c < nv) {       // vertical filter c: t ascending, d ascending
        float acc = first ? W[(long)Dx * T * nv + c] : po[c];
        for (int t = t0; t < tend; ++t) {
          const float* xr = xs + (t - t0) * Dx;
          const float* w = W + (long)t * nv + c;
          for (int d = 0; d < Dx; d += 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(xr + d);
            acc = fmaf(x.x, w[(long)d * T * nv], acc);
            acc = fmaf(x.y, w[(long)(d + 1) * T * nv], acc);
            acc = fmaf(x.z, w[(long)(d + 2) * T * nv], acc);
            acc = fmaf(x.w, w[(long)(d + 3) * T * nv], acc);
          }
        }
        po[c] = last ? fmaxf(acc, 0.f) : acc;
        continue;
      }
      const int h = (c - nv) / nh + 1, f = (c - nv) - (h - 1) * nh;
      const float* __restrict__ wh = W + cz_hoff(T, Dx, nv, nh, h);
      const float bias = wh[(long)h * Dx * nh + f];
      float best = first ? -INFINITY : po[c];
      int arg = first ? 0 : amax[c - nv];
      int* __restrict__ tw = ties + (long)(c - nv) * TS;
      int ntie = first ? 0 : tw[0];
      const int pend = min(t0 + CH, T - h + 1);       // positions of this chunk that have a whole window
      for (int p = t0; p < pend; p += CZ_TC) {
        float acc[CZ_TC];
#pragma unroll
        for (int i = 0; i < CZ_TC; ++i) acc[i] = bias;
        for (int j = 0; j < h; ++j) {
          const float* xr = xs + (p - t0 + j) * Dx;
          const float* w = wh + (long)j * Dx * nh + f;
          for (int d = 0; d < Dx; d += 4) {
            const float w0 = w[(long)d * nh], w1 = w[(long)(d + 1) * nh], w2 = w[(long)(d + 2) * nh],
                        w3 = w[(long)(d + 3) * nh];
#pragma unroll
            for (int i = 0; i < CZ_TC; ++i) {       // (rows past the chunk's last window are zero-filled or unused)
              const f32x4 x = *reinterpret_cast<const f32x4*>(xr + i * Dx + d);
              acc[i] = fmaf(x.x, w0, acc[i]);
              acc[i] = fmaf(x.y, w1, acc[i]);
              acc[i] = fmaf(x.z, w2, acc[i]);
              acc[i] = fmaf(x.w, w3, acc[i]);
            }
          }
        }
        // (a tile never straddles a mask word: p is a multiple of CZ_TC, which divides 32)
        unsigned cur = (p & 31) ? (unsigned)tw[1 + (p >> 5)] : 0u;
#pragma unroll
        for (int i = 0; i < CZ_TC; ++i) {
          if (p + i < pend) {
            const unsigned bit = 1u << ((p + i) & 31);
            if (acc[i] > best) {        // strict: arg is the FIRST maximum; the ties start again with it
              best = acc[i];
              arg = p + i;
              ntie = 1;
              cur = bit;
            } else if (acc[i] == best) {
              ++ntie;
              cur |= bit;
            }
          }
        }
        tw[1 + (p >> 5)] = (int)cur;
      }
      po[c] = last ? fmaxf(best, 0.f) : best;
      amax[c - nv] = arg;
      tw[0] = ntie;
    }
  }
}

extern "C" int clsr_caser_hconv_fwd(const float* hist, int ldh, long Hn, int T, int Di, int Dc, const float* Wi,
                                    const float* Wc, int L, int n_v, int n_h, float* pooled, int ldp, int* argmax_i,
                                    int* argmax_c, int* ties_i, int* ties_c, void* stream) {
  CLSR_CHECK_ARG(hist && Wi && Wc && pooled && argmax_i && argmax_c && ties_i && ties_c);
  CLSR_CHECK_ARG(Hn >= 0 && T > 0 && Di > 0 && Dc > 0);
  CLSR_CHECK_ARG(L >= 1 && L <= T && n_v > 0 && n_h > 0);
  CLSR_CHECK_SUPPORTED(clsr_caser_supported(T, Di, Dc, L, n_v, n_h));
  CLSR_CHECK_ARG(ldh >= Di + Dc && ldh % 4 == 0 && ldp >= 2 * (n_v + L * n_h));
  CLSR_CHECK_SUPPORTED(((uintptr_t)hist % 16) == 0 && Hn < (1L << 31));
  if (Hn == 0) return CLSR_OK;
  const int CH = cz_chunk(T, Di, Dc, L), Dm = Di > Dc ? Di : Dc;
  const size_t shmem = (size_t)(CH + L - 1) * Dm * sizeof(float);      // <= 64 KB (cz_chunk)
  hipLaunchKernelGGL(caser_fwd_kernel, dim3((unsigned)Hn, 2), dim3(256), shmem, (hipStream_t)stream, hist, ldh, T, Di,
                     Dc, Wi, Wc, L, n_v, n_h, CH, pooled, ldp, argmax_i, argmax_c, ties_i, ties_c);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ------------------------------------------------------------------------------------------------ backward
// g = d pooled where the pooled value is positive (the ReLU gate), 0 elsewhere.
//
// d hist: one workgroup per (history, table); the gated gradients and the first-maximum positions of the history sit in
// LDS, a thread owns (t, d) elements and walks every filter in ascending order:
//   d hist[b, t, d] += sum_f g_v[f] Wv[d, t, f]
//                      + sum_h sum_f sum_{s tied in pool (h, f), 0 <= t - s < h} g[h, f] / n(h, f) * Wh_h[t - s, d, f]
// (n: the pool's number of tied positions; one of them -- the rule -- is the fast path).
// LDS (4-byte words): g / n [PW] | first maximum [L * nh] | n [L * nh]
__global__ void __launch_bounds__(256) caser_bwd_hist_kernel(const float* __restrict__ dpool, int ldd,
                                                            const float* __restrict__ pooled, int ldp,
                                                            const int* __restrict__ amax_i,
                                                            const int* __restrict__ amax_c,
                                                            const int* __restrict__ ties_i,
                                                            const int* __restrict__ ties_c, int T, int Di, int Dc,
                                                            const float* __restrict__ Wi, const float* __restrict__ Wc,
                                                            int L, int nv, int nh, float* __restrict__ dhist, int ldh) {
  extern __shared__ __attribute__((aligned(16))) float gs[];
  const int tab = blockIdx.y, tid = threadIdx.x;
  const long b = blockIdx.x;
  const int Dx = tab ? Dc : Di, col0 = tab ? Di : 0;
  const float* __restrict__ W = tab ? Wc : Wi;
  const int* __restrict__ amax = (tab ? amax_c : amax_i) + b * L * nh;
  const int TS = 1 + ((T + 31) >> 5);
  const int* __restrict__ ties = (tab ? ties_c : ties_i) + b * L * nh * TS;
  const int PW = nv + L * nh;
  int* ts = reinterpret_cast<int*>(gs + PW);
  int* ns = ts + L * nh;
  for (int c = tid; c < PW; c += 256) {
    const float g = pooled[b * ldp + (long)tab * PW + c] > 0.f ? dpool[b * ldd + (long)tab * PW + c] : 0.f;
    if (c < nv) {
      gs[c] = g;
      continue;
    }
    const int n = g != 0.f ? ties[(long)(c - nv) * TS] : 1;
    gs[c] = n > 1 ? g * (1.0f / (float)n) : g;
    ts[c - nv] = g != 0.f ? amax[c - nv] : -(1 << 30);      // (a closed pool matches no position)
    ns[c - nv] = n;
  }
  __syncthreads();
  for (int e = tid; e < T * Dx; e += 256) {
    const int t = e / Dx, d = e - t * Dx;
    float acc = 0.f;
    const float* wv = W + ((long)d * T + t) * nv;
    for (int f = 0; f < nv; f += 4) {       // (n_v % 4 == 0: rows of Wv and g are 16-byte aligned)
      const f32x4 g = *reinterpret_cast<const f32x4*>(gs + f);
      const f32x4 w = *reinterpret_cast<const f32x4*>(wv + f);
      acc = fmaf(g.x, w.x, acc);
      acc = fmaf(g.y, w.y, acc);
      acc = fmaf(g.z, w.z, acc);
      acc = fmaf(g.w, w.w, acc);
    }
    for (int h = 1; h <= L; ++h) {
      const float* wh = W + cz_hoff(T, Dx, nv, nh, h) + (long)d * nh;
      const float* gh = gs + nv + (h - 1) * nh;
      const int* th = ts + (h - 1) * nh;
      const int* nt = ns + (h - 1) * nh;
      for (int f = 0; f < nh; ++f) {
        const int j = t - th[f];        // offset of t in the window at the first maximum
        if (nt[f] == 1) {
          if ((unsigned)j < (unsigned)h) acc = fmaf(gh[f], wh[(long)j * Dx * nh + f], acc);
        } else if (j >= 0) {            // every tied window that covers t, nearest first
          const int* tw = ties + ((long)(h - 1) * nh + f) * TS + 1;
          for (int jj = 0; jj < h && jj <= j; ++jj) {
            const int s = t - jj;
            if (s <= T - h && (((unsigned)tw[s >> 5] >> (s & 31)) & 1u)) acc = fmaf(gh[f], wh[(long)jj * Dx * nh + f], acc);
          }
        }
      }
    }
    dhist[(b * T + t) * ldh + col0 + d] += acc;
  }
}

// Weight and bias gradients: a thread owns one element of the table's gradient block and sums over the histories of its
// slice (blockIdx.y) in ascending order:
//   dWv[d, t, f] = sum_b g_v[b, f] X[b, t, d]          dWh_h[j, d, f] = sum_b g[b, h, f] X[b, t*(b, h, f) + j, d]
//   dbv[f] = sum_b g_v[b, f]                           dbh_h[f] = sum_b g[b, h, f]
// (a gathered sum: the selected window differs per filter; a pool with n tied positions: the mean of their windows).
// out: the slice's row of the workspace, or -- one slice -- the gradient block itself.
__global__ void __launch_bounds__(256) caser_bwd_w_kernel(const float* __restrict__ dpool, int ldd,
                                                         const float* __restrict__ pooled, int ldp,
                                                         const int* __restrict__ amax_i, const int* __restrict__ amax_c,
                                                         const int* __restrict__ ties_i, const int* __restrict__ ties_c,
                                                         const float* __restrict__ hist, int ldh, long Hn, int T,
                                                         int Di, int Dc, int L, int nv, int nh, long Si, long Sc,
                                                         long slice, float* __restrict__ out_i,
                                                         float* __restrict__ out_c, long out_stride) {
  const int tab = blockIdx.z;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (tab ? Sc : Si)) return;
  const int Dx = tab ? Dc : Di, col0 = tab ? Di : 0;
  const int* __restrict__ amax = tab ? amax_c : amax_i;
  const int* __restrict__ ties = tab ? ties_c : ties_i;
  const int TS = 1 + ((T + 31) >> 5);
  const int PW = nv + L * nh;
  int hh = 1;       // width of the element's filter (horizontal kernels)
  // decode the element: pooled column c, window offset j (-1: bias, -2: vertical kernel at position t), input column d
  int c, j, d = 0, t = 0;
  const long nvk = (long)Dx * T * nv;
  if (e < nvk) {
    d = (int)(e / ((long)T * nv));
    const long r = e - (long)d * T * nv;
    t = (int)(r / nv);
    c = (int)(r - (long)t * nv);
    j = -2;
  } else if (e < nvk + nv) {
    c = (int)(e - nvk);
    j = -1;
  } else {
    long r = e - nvk - nv;
    int h = 1;
    while (r >= cz_hblock(Dx, h, nh)) {
      r -= cz_hblock(Dx, h, nh);
      ++h;
    }
    const long nk = (long)h * Dx * nh;
    hh = h;
    if (r < nk) {
      j = (int)(r / ((long)Dx * nh));
      const long q = r - (long)j * Dx * nh;
      d = (int)(q / nh);
      c = nv + (h - 1) * nh + (int)(q - (long)d * nh);
    } else {
      c = nv + (h - 1) * nh + (int)(r - nk);
      j = -1;
    }
  }
  const long b0 = blockIdx.y * slice, b1 = min(Hn, b0 + slice);
  const long pc = (long)tab * PW + c;
  float acc = 0.f;
  for (long b = b0; b < b1; ++b) {
    const float g = pooled[b * ldp + pc] > 0.f ? dpool[b * ldd + pc] : 0.f;
    if (j == -1) {
      acc += g;
    } else if (j == -2) {
      acc = fmaf(g, hist[(b * T + t) * ldh + col0 + d], acc);
    } else if (g != 0.f) {
      const long q = b * L * nh + (c - nv);
      const int a = amax[q], n = ties[q * TS];
      if (n == 1) {
        acc = fmaf(g, hist[(b * T + a + j) * ldh + col0 + d], acc);
      } else {
        const float gn = g * (1.0f / (float)n);
        for (int s = a; s <= T - hh; ++s)
          if (((unsigned)ties[q * TS + 1 + (s >> 5)] >> (s & 31)) & 1u)
            acc = fmaf(gn, hist[(b * T + s + j) * ldh + col0 + d], acc);
      }
    }
  }
  (tab ? out_c : out_i)[(long)blockIdx.y * out_stride + e] = acc;
}

// gradient block = sum of the slices' partial rows, slice 0 first
__global__ void __launch_bounds__(256) caser_bwd_w_reduce_kernel(const float* __restrict__ ws, int parts, long Si,
                                                                long Sc, float* __restrict__ dWi,
                                                                float* __restrict__ dWc) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x, S = Si + Sc;
  if (e >= S) return;
  float s = ws[e];
  for (int p = 1; p < parts; ++p) s += ws[(long)p * S + e];
  if (e < Si) dWi[e] = s;
  else dWc[e - Si] = s;
}

// slices of the history range the weight-gradient partial sums are split into
extern "C" int clsr_caser_hconv_bwd_parts(long Hn, int T, int Di, int Dc, int L, int n_v, int n_h) {
  if (Hn <= 0 || !clsr_caser_supported(T, Di, Dc, L, n_v, n_h)) return 0;
  const long S = cz_block(T, Di, L, n_v, n_h) + cz_block(T, Dc, L, n_v, n_h);
  long parts = CZ_WS_FLOATS / S;
  if (parts > 16) parts = 16;
  if (parts > Hn) parts = Hn;
  return parts < 1 ? 1 : (int)parts;
}

extern "C" long clsr_caser_hconv_bwd_workspace_floats(long Hn, int T, int Di, int Dc, int L, int n_v, int n_h) {
  const int parts = clsr_caser_hconv_bwd_parts(Hn, T, Di, Dc, L, n_v, n_h);
  if (parts <= 1) return 4;       // (one slice writes the gradient block itself)
  return parts * (cz_block(T, Di, L, n_v, n_h) + cz_block(T, Dc, L, n_v, n_h));
}

extern "C" int clsr_caser_hconv_bwd(const float* dpool, int ldd, const float* pooled, int ldp, const int* argmax_i,
                                    const int* argmax_c, const int* ties_i, const int* ties_c, const float* hist,
                                    int ldh, long Hn, int T, int Di, int Dc, const float* Wi, const float* Wc, int L,
                                    int n_v, int n_h, float* dhist, float* dWi, float* dWc, float* workspace,
                                    void* stream) {
  CLSR_CHECK_ARG(dpool && pooled && argmax_i && argmax_c && ties_i && ties_c && hist);
  CLSR_CHECK_ARG(Wi && Wc && dhist && dWi && dWc && workspace);
  CLSR_CHECK_ARG(Hn > 0 && T > 0 && Di > 0 && Dc > 0 && L >= 1 && L <= T && n_v > 0 && n_h > 0);
  CLSR_CHECK_SUPPORTED(clsr_caser_supported(T, Di, Dc, L, n_v, n_h) && Hn < (1L << 31));
  const int PW = n_v + L * n_h;
  CLSR_CHECK_ARG(ldh >= Di + Dc && ldd >= 2 * PW && ldp >= 2 * PW);
  hipStream_t s = (hipStream_t)stream;
  const size_t shmem = (size_t)(PW + 2 * L * n_h) * sizeof(float);      // <= 64 KB (clsr_caser_supported)
  hipLaunchKernelGGL(caser_bwd_hist_kernel, dim3((unsigned)Hn, 2), dim3(256), shmem, s, dpool, ldd, pooled, ldp,
                     argmax_i, argmax_c, ties_i, ties_c, T, Di, Dc, Wi, Wc, L, n_v, n_h, dhist, ldh);
  CLSR_CHECK_LAUNCH();
  const long Si = cz_block(T, Di, L, n_v, n_h), Sc = cz_block(T, Dc, L, n_v, n_h);
  const int parts = clsr_caser_hconv_bwd_parts(Hn, T, Di, Dc, L, n_v, n_h);
  const long slice = (Hn + parts - 1) / parts;
  const dim3 grid(clsr_cdiv(Si > Sc ? Si : Sc, 256), parts, 2);
  if (parts == 1) {
    hipLaunchKernelGGL(caser_bwd_w_kernel, grid, dim3(256), 0, s, dpool, ldd, pooled, ldp, argmax_i, argmax_c, ties_i,
                       ties_c, hist, ldh, Hn, T, Di, Dc, L, n_v, n_h, Si, Sc, slice, dWi, dWc, 0L);
    CLSR_CHECK_LAUNCH();
    return CLSR_OK;
  }
  hipLaunchKernelGGL(caser_bwd_w_kernel, grid, dim3(256), 0, s, dpool, ldd, pooled, ldp, argmax_i, argmax_c, ties_i, ties_c,
                     hist, ldh, Hn, T, Di, Dc, L, n_v, n_h, Si, Sc, slice, workspace, workspace + Si, Si + Sc);
  CLSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(caser_bwd_w_reduce_kernel, dim3(clsr_cdiv(Si + Sc, 256)), dim3(256), 0, s, workspace, parts, Si,
                     Sc, dWi, dWc);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}
