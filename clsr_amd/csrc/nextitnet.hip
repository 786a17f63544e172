// NextItNet (models/sequential/nextitnet.py): the stack of residual blocks between the history gather and model_output,
// over x_0 = hist [Hn, T, C] (C = Di + Dc, half = C / 2), one block per entry of dilations (rate d, width k):
//
//   a1 = relu(LN1(x))                 z1 = a1 . W1 + b1                                       [T, half]
//   a2 = relu(LN2(z1))                z2[t] = bd + sum_{j < k} a2[t - (k - 1 - j) d] . Wd[j]   [T, half]  (t - .. < 0: zero)
//   a3 = relu(LN3(z2))                x'  = x + a3 . W2 + b2                                  [T, C]
//   LN(v) = gamma * (v - mean) / sqrt(var + 1e-8) + beta over the channel axis, biased variance; relu open for > 0 only.
//
// NO mask: padded steps (embedding row 0, histories are left-padded) take part like every other, as in the reference.
//
// Parameter block of ONE residual block (floats; the order the reference creates the variables in, each contiguous):
//   beta1 [C] | gamma1 [C] | W1 [C][half] | b1 [half] | beta2 [half] | gamma2 [half] | Wd [k][half][half] | bd [half] |
//   beta3 [half] | gamma3 [half] | W2 [half][C] | b2 [C]
// = 3 C + 2 C half + 6 half + k half^2 floats; C is a multiple of 8, so every tensor starts 16-byte aligned and the block
// has no padding.  The blocks follow one another; the gradient block has the same layout.
//
// Work split: a workgroup of 256 threads owns a SLICE of S = min(256 / T, what LDS holds) histories at a time and walks
// slices in a persistent loop; thread s * T + t owns position t of the slice's history s.  A history's activations stay in
// LDS from block to block (row strides C + 1 and half + 1 words: a wave's 64 rows hit 64 banks); the weights are read at
// wave-uniform addresses (scalar loads, four outputs per load).  fp32 FMA chains in a fixed order per output element.
//   forward   LDS per history: T (C + 1) + 2 T (half + 1) words.
//   backward  LDS per history: 2 T (C + 1) + 3 T (half + 1) words, plus 8 C words per workgroup.  It recomputes a block
//             from its saved input x_l (the ONLY training state: nothing else is saved), then walks the block backwards.
//             Weight, bias, gamma and beta gradients are summed over the slice's rows by one owner thread per element
//             (gamma1 / beta1: a wave reduction, the four waves added in ascending order) into the workgroup's row of
//             partial sums; the caller reduces the rows in ascending order.  No atomics: two runs are bit-identical.
// Both kernels stay within 64 KB of LDS per workgroup (clsr_nextitnet_supported says so for the backward, the larger).
#include "common.h"

#define NX_THREADS 256
#define NX_LDS_FLOATS 16384          // 64 KB per workgroup
#define NX_MAX_C 128
#define NX_MAX_K 8
#define NX_MAX_BLOCKS 16
#define NX_MAX_PARTS 512
#define NX_WS_FLOATS (1L << 24)
#define NX_EPS 1e-8f

__host__ __device__ static inline long nx_block_floats(int C, int k) {
  const long h = C / 2;
  return 3L * C + 2L * C * h + 6L * h + (long)k * h * h;
}
static inline long nx_fwd_hist_floats(int T, int C) { return (long)T * (C + 1) + 2L * T * (C / 2 + 1); }
static inline long nx_bwd_hist_floats(int T, int C) { return 2L * T * (C + 1) + 3L * T * (C / 2 + 1); }
static inline long nx_bwd_fixed_floats(int C) { return 8L * C; }

static int nx_slice(int T, int C, int training) {
  const long per = training ? nx_bwd_hist_floats(T, C) : nx_fwd_hist_floats(T, C);
  const long room = NX_LDS_FLOATS - (training ? nx_bwd_fixed_floats(C) : 0);
  long s = room / per;
  if (s > NX_THREADS / T) s = NX_THREADS / T;
  return (int)s;
}

extern "C" int clsr_nextitnet_max_channels(void) { return NX_MAX_C; }
extern "C" int clsr_nextitnet_max_kernel(void) { return NX_MAX_K; }
extern "C" int clsr_nextitnet_max_blocks(void) { return NX_MAX_BLOCKS; }
extern "C" long clsr_nextitnet_lds_budget_bytes(void) { return 4L * NX_LDS_FLOATS; }

// LDS bytes of a slice of ONE history (training: the backward, which is the larger)
extern "C" long clsr_nextitnet_lds_bytes(int T, int C, int training) {
  if (T <= 0 || C <= 0) return 0;
  return 4L * (training ? nx_bwd_hist_floats(T, C) + nx_bwd_fixed_floats(C) : nx_fwd_hist_floats(T, C));
}

extern "C" int clsr_nextitnet_supported(int T, int C, int k, int nblocks, int max_dilation) {
  if (T <= 0 || T > 256 || C <= 0 || C % 8 || C > NX_MAX_C) return 0;
  if (k < 1 || k > NX_MAX_K || nblocks < 1 || nblocks > NX_MAX_BLOCKS || max_dilation < 1) return 0;
  return clsr_nextitnet_lds_bytes(T, C, 1) <= clsr_nextitnet_lds_budget_bytes();
}

extern "C" long clsr_nextitnet_param_floats(int C, int k, int nblocks) {
  if (C <= 0 || C % 8 || k < 1 || nblocks < 1) return 0;
  return nblocks * nx_block_floats(C, k);
}

// histories a workgroup holds at a time (training: the backward)
extern "C" int clsr_nextitnet_slice(int T, int C, int training) {
  if (T <= 0 || T > 256 || C <= 0 || C % 8 || C > NX_MAX_C) return 0;
  return nx_slice(T, C, training);
}

// workgroups of the backward = rows of partial sums
extern "C" int clsr_nextitnet_parts(long Hn, int T, int C, int k, int nblocks) {
  if (Hn <= 0 || !clsr_nextitnet_supported(T, C, k, nblocks, 1)) return 0;
  const int S = nx_slice(T, C, 1);
  long parts = (Hn + S - 1) / S;
  if (parts > NX_MAX_PARTS) parts = NX_MAX_PARTS;
  const long cap = NX_WS_FLOATS / clsr_nextitnet_param_floats(C, k, nblocks);
  if (parts > cap) parts = cap;
  return parts < 1 ? 1 : (int)parts;
}

extern "C" long clsr_nextitnet_workspace_floats(long Hn, int T, int C, int k, int nblocks) {
  return clsr_nextitnet_parts(Hn, T, C, k, nblocks) * clsr_nextitnet_param_floats(C, k, nblocks);
}

// ------------------------------------------------------------------------------------------------ device helpers
struct NxOff {
  int be1, g1, W1, b1, be2, g2, Wd, bd, be3, g3, W2, b2;
};
__device__ __forceinline__ NxOff nx_offsets(int C, int k) {
  const int h = C >> 1;
  NxOff o;
  o.be1 = 0;
  o.g1 = C;
  o.W1 = 2 * C;
  o.b1 = o.W1 + C * h;
  o.be2 = o.b1 + h;
  o.g2 = o.be2 + h;
  o.Wd = o.g2 + h;
  o.bd = o.Wd + k * h * h;
  o.be3 = o.bd + h;
  o.g3 = o.be3 + h;
  o.W2 = o.g3 + h;
  o.b2 = o.W2 + h * C;
  return o;
}

// mean and 1 / sqrt(biased variance + eps) of v[0 .. n)
__device__ __forceinline__ void nx_stats(const float* v, int n, float& mean, float& rstd) {
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
  rstd = 1.0f / sqrtf(q / (float)n + NX_EPS);
}

// acc[q] += sum_n v[n] * W[n * ld + q], n < N (W: wave-uniform address)
__device__ __forceinline__ void nx_axpy4(const float* v, const float* __restrict__ W, int ld, int N, f32x4& acc) {
#pragma unroll 4
  for (int n = 0; n < N; ++n) {      // (several wave-uniform weight loads in flight: the chain per accumulator keeps its order)
    const float x = v[n];
    const f32x4 w = ld4(W + (long)n * ld);
    acc.x = fmaf(x, w.x, acc.x);
    acc.y = fmaf(x, w.y, acc.y);
    acc.z = fmaf(x, w.z, acc.z);
    acc.w = fmaf(x, w.w, acc.w);
  }
}

// acc[q] += sum_n v[n] * W[q * ld + n], n < N (a multiple of 4)
__device__ __forceinline__ void nx_dot4(const float* v, const float* __restrict__ W, int ld, int N, f32x4& acc) {
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

__device__ __forceinline__ float nx_relu(float v) { return v > 0.f ? v : 0.f; }

// ------------------------------------------------------------------------------------------------ forward
// saved (training) [nb][Hn][T][C]: the input of every block.  out: row ((h T + t) rep + g) (all positions) or (h rep + g)
// (last_only: position T - 1), g < rep, ldo floats apart, columns 0 .. C.
__global__ void __launch_bounds__(NX_THREADS) nx_fwd_kernel(const float* __restrict__ hist, long Hn, int T, int C,
                                                            const float* __restrict__ params, int k, int nb,
                                                            const int* __restrict__ dil, float* __restrict__ saved,
                                                            float* __restrict__ out, int ldo, int rep, int last_only,
                                                            int S) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, h = C >> 1, LX = C + 1, LH = h + 1;
  float* X = lds;
  float* A = X + S * T * LX;
  float* Bf = A + S * T * LH;
  const NxOff of = nx_offsets(C, k);
  const long PB = nx_block_floats(C, k);
  const int t = tid % T;
  for (long base = (long)blockIdx.x * S; base < Hn; base += (long)gridDim.x * S) {
    const int nact = (int)min((long)S, Hn - base), rows = nact * T;
    const bool active = tid < rows;
    const float* __restrict__ src = hist + base * T * C;
    __syncthreads();
    for (int e = tid; e < rows * C; e += NX_THREADS) {
      const int r = e / C;
      X[r * LX + (e - r * C)] = src[e];
    }
    __syncthreads();
    float* xr = X + tid * LX;
    float* ar = A + tid * LH;
    float* br = Bf + tid * LH;
    for (int l = 0; l < nb; ++l) {
      const float* __restrict__ p = params + l * PB;
      const long d = dil[l];
      if (saved) {
        float* __restrict__ dst = saved + ((long)l * Hn + base) * T * C;
        for (int e = tid; e < rows * C; e += NX_THREADS) {
          const int r = e / C;
          dst[e] = X[r * LX + (e - r * C)];
        }
      }
      if (active) {
        float mean, rstd;
        nx_stats(xr, C, mean, rstd);
        for (int o = 0; o < h; o += 4) {
          f32x4 acc = ld4(p + of.b1 + o);
#pragma unroll 4
          for (int c = 0; c < C; ++c) {
            const float a = nx_relu(fmaf(p[of.g1 + c], (xr[c] - mean) * rstd, p[of.be1 + c]));
            const f32x4 w = ld4(p + of.W1 + c * h + o);
            acc.x = fmaf(a, w.x, acc.x);
            acc.y = fmaf(a, w.y, acc.y);
            acc.z = fmaf(a, w.z, acc.z);
            acc.w = fmaf(a, w.w, acc.w);
          }
          ar[o] = acc.x, ar[o + 1] = acc.y, ar[o + 2] = acc.z, ar[o + 3] = acc.w;
        }
        nx_stats(ar, h, mean, rstd);
        for (int i = 0; i < h; ++i) ar[i] = nx_relu(fmaf(p[of.g2 + i], (ar[i] - mean) * rstd, p[of.be2 + i]));
      }
      __syncthreads();
      if (active) {
        for (int o = 0; o < h; o += 4) {
          f32x4 acc = ld4(p + of.bd + o);
          for (int j = 0; j < k; ++j) {
            const long off = (long)(k - 1 - j) * d;
            if (off > t) continue;          // (the tap reads the zero padding)
            nx_axpy4(ar - off * LH, p + of.Wd + (long)j * h * h + o, h, h, acc);
          }
          br[o] = acc.x, br[o + 1] = acc.y, br[o + 2] = acc.z, br[o + 3] = acc.w;
        }
        float mean, rstd;
        nx_stats(br, h, mean, rstd);
        for (int i = 0; i < h; ++i) br[i] = nx_relu(fmaf(p[of.g3 + i], (br[i] - mean) * rstd, p[of.be3 + i]));
        for (int c = 0; c < C; c += 4) {
          f32x4 acc = ld4(p + of.b2 + c);
          nx_axpy4(br, p + of.W2 + c, C, h, acc);
          xr[c] += acc.x, xr[c + 1] += acc.y, xr[c + 2] += acc.z, xr[c + 3] += acc.w;
        }
      }
      __syncthreads();
    }
    if (last_only) {
      for (int e = tid; e < nact * rep * C; e += NX_THREADS) {
        const int row = e / C, c = e - row * C, s = row / rep;
        out[(base * rep + row) * ldo + c] = X[(s * T + T - 1) * LX + c];
      }
    } else {
      for (int e = tid; e < rows * rep * C; e += NX_THREADS) {
        const int row = e / C, c = e - row * C, r = row / rep;
        out[(base * T * rep + row) * ldo + c] = X[r * LX + c];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
__device__ __forceinline__ void nx_acc(float* __restrict__ g, bool first, float v) { *g = first ? v : *g + v; }

__global__ void __launch_bounds__(NX_THREADS) nx_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ saved,
                                                            long Hn, int T, int C, const float* __restrict__ params,
                                                            int k, int nb, const int* __restrict__ dil,
                                                            float* __restrict__ dhist, float* __restrict__ partial,
                                                            int S) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, h = C >> 1, LX = C + 1, LH = h + 1;
  float* X = lds;                       // xhat1 of the block's input
  float* G = X + S * T * LX;            // gradient w.r.t. the block's output, then its input
  float* A = G + S * T * LX;            // xhat2
  float* Bf = A + S * T * LH;           // xhat3, then d u2, then d z1
  float* Cb = Bf + S * T * LH;          // d u3, then d z2
  float* red = Cb + S * T * LH;         // [4 waves][2 C]
  const NxOff of = nx_offsets(C, k);
  const long PB = nx_block_floats(C, k);
  const int t = tid % T, wave = tid >> 6, lane = tid & 63;
  const float invC = 1.0f / (float)C, invh = 1.0f / (float)h;
  float* __restrict__ part = partial + (long)blockIdx.x * nb * PB;
  bool first = true;
  for (long base = (long)blockIdx.x * S; base < Hn; base += (long)gridDim.x * S, first = false) {
    const int nact = (int)min((long)S, Hn - base), rows = nact * T;
    const bool active = tid < rows;
    const int row = active ? tid : 0;
    float* xr = X + row * LX;
    float* gr = G + row * LX;
    float* ar = A + row * LH;
    float* br = Bf + row * LH;
    float* cr = Cb + row * LH;
    __syncthreads();
    {
      const float* __restrict__ src = dout + base * T * C;
      for (int e = tid; e < rows * C; e += NX_THREADS) {
        const int r = e / C;
        G[r * LX + (e - r * C)] = src[e];
      }
    }
    for (int l = nb - 1; l >= 0; --l) {
      const float* __restrict__ p = params + l * PB;
      float* __restrict__ gp = part + l * PB;
      const long d = dil[l];
      __syncthreads();
      {
        const float* __restrict__ src = saved + ((long)l * Hn + base) * T * C;
        for (int e = tid; e < rows * C; e += NX_THREADS) {
          const int r = e / C;
          X[r * LX + (e - r * C)] = src[e];
        }
      }
      __syncthreads();
      // ---- the block again: xhat1 -> X, xhat2 -> A
      float rstd1 = 0.f, rstd2 = 0.f, rstd3 = 0.f;
      if (active) {
        float mean;
        nx_stats(xr, C, mean, rstd1);
        for (int c = 0; c < C; ++c) xr[c] = (xr[c] - mean) * rstd1;
        for (int o = 0; o < h; o += 4) {
          f32x4 acc = ld4(p + of.b1 + o);
#pragma unroll 4
          for (int c = 0; c < C; ++c) {
            const float a = nx_relu(fmaf(p[of.g1 + c], xr[c], p[of.be1 + c]));
            const f32x4 w = ld4(p + of.W1 + c * h + o);
            acc.x = fmaf(a, w.x, acc.x);
            acc.y = fmaf(a, w.y, acc.y);
            acc.z = fmaf(a, w.z, acc.z);
            acc.w = fmaf(a, w.w, acc.w);
          }
          ar[o] = acc.x, ar[o + 1] = acc.y, ar[o + 2] = acc.z, ar[o + 3] = acc.w;
        }
        nx_stats(ar, h, mean, rstd2);
        for (int i = 0; i < h; ++i) ar[i] = (ar[i] - mean) * rstd2;
      }
      __syncthreads();
      // ---- xhat3 -> Bf
      if (active) {
        for (int o = 0; o < h; o += 4) {
          f32x4 acc = ld4(p + of.bd + o);
          for (int j = 0; j < k; ++j) {
            const long off = (long)(k - 1 - j) * d;
            if (off > t) continue;
            const float* an = ar - off * LH;
            const float* __restrict__ W = p + of.Wd + (long)j * h * h + o;
#pragma unroll 4
            for (int i = 0; i < h; ++i) {
              const float a = nx_relu(fmaf(p[of.g2 + i], an[i], p[of.be2 + i]));
              const f32x4 w = ld4(W + i * h);
              acc.x = fmaf(a, w.x, acc.x);
              acc.y = fmaf(a, w.y, acc.y);
              acc.z = fmaf(a, w.z, acc.z);
              acc.w = fmaf(a, w.w, acc.w);
            }
          }
          br[o] = acc.x, br[o + 1] = acc.y, br[o + 2] = acc.z, br[o + 3] = acc.w;
        }
        float mean;
        nx_stats(br, h, mean, rstd3);
        for (int i = 0; i < h; ++i) br[i] = (br[i] - mean) * rstd3;
        // ---- d u3 = gate3 (G . W2^T) -> Cb
        for (int o = 0; o < h; o += 4) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          nx_dot4(gr, p + of.W2 + o * C, C, C, acc);
          const float da[4] = {acc.x, acc.y, acc.z, acc.w};
          for (int q = 0; q < 4; ++q)
            cr[o + q] = fmaf(p[of.g3 + o + q], br[o + q], p[of.be3 + o + q]) > 0.f ? da[q] : 0.f;
        }
      }
      __syncthreads();
      // ---- d W2, d b2, d gamma3, d beta3 (one owner thread per element, rows ascending)
      for (int e = tid; e < h * C; e += NX_THREADS) {
        const int o = e / C, c = e - o * C;
        const float g = p[of.g3 + o], b = p[of.be3 + o];
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s = fmaf(nx_relu(fmaf(g, Bf[r * LH + o], b)), G[r * LX + c], s);
        nx_acc(gp + of.W2 + e, first, s);
      }
      for (int c = tid; c < C; c += NX_THREADS) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += G[r * LX + c];
        nx_acc(gp + of.b2 + c, first, s);
      }
      for (int o = tid; o < h; o += NX_THREADS) {
        float sg = 0.f, sb = 0.f;
        for (int r = 0; r < rows; ++r) {
          const float du = Cb[r * LH + o];
          sg = fmaf(du, Bf[r * LH + o], sg);
          sb += du;
        }
        nx_acc(gp + of.g3 + o, first, sg);
        nx_acc(gp + of.be3 + o, first, sb);
      }
      __syncthreads();
      // ---- d z2 = LN3 backward, in place in Cb
      if (active) {
        float s1 = 0.f, s2 = 0.f;
        for (int o = 0; o < h; ++o) {
          const float dx = cr[o] * p[of.g3 + o];
          s1 += dx;
          s2 = fmaf(dx, br[o], s2);
        }
        s1 *= invh, s2 *= invh;
        for (int o = 0; o < h; ++o) cr[o] = rstd3 * (cr[o] * p[of.g3 + o] - s1 - br[o] * s2);
      }
      __syncthreads();
      // ---- d u2 = gate2 (sum_j d z2[t + (k - 1 - j) d] . Wd[j]^T) -> Bf
      if (active) {
        for (int i = 0; i < h; i += 4) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          for (int j = 0; j < k; ++j) {
            const long off = (long)(k - 1 - j) * d;
            if (t + off >= T) continue;
            nx_dot4(cr + off * LH, p + of.Wd + ((long)j * h + i) * h, h, h, acc);
          }
          const float da[4] = {acc.x, acc.y, acc.z, acc.w};
          for (int q = 0; q < 4; ++q)
            br[i + q] = fmaf(p[of.g2 + i + q], ar[i + q], p[of.be2 + i + q]) > 0.f ? da[q] : 0.f;
        }
      }
      __syncthreads();
      // ---- d Wd, d bd, d gamma2, d beta2
      for (int e = tid; e < k * h * h; e += NX_THREADS) {
        const int j = e / (h * h), i = (e - j * h * h) / h, o = e - (j * h + i) * h;
        const long off = (long)(k - 1 - j) * d;
        const float g = p[of.g2 + i], b = p[of.be2 + i];
        float s = 0.f;
        if (off < T) {
          const int o_ = (int)off;
          for (int hs = 0; hs < nact; ++hs)
            for (int tt = o_; tt < T; ++tt)
              s = fmaf(nx_relu(fmaf(g, A[(hs * T + tt - o_) * LH + i], b)), Cb[(hs * T + tt) * LH + o], s);
        }
        nx_acc(gp + of.Wd + e, first, s);
      }
      for (int o = tid; o < h; o += NX_THREADS) {
        float sd = 0.f, sg = 0.f, sb = 0.f;
        for (int r = 0; r < rows; ++r) {
          sd += Cb[r * LH + o];
          const float du = Bf[r * LH + o];
          sg = fmaf(du, A[r * LH + o], sg);
          sb += du;
        }
        nx_acc(gp + of.bd + o, first, sd);
        nx_acc(gp + of.g2 + o, first, sg);
        nx_acc(gp + of.be2 + o, first, sb);
      }
      __syncthreads();
      // ---- d z1 = LN2 backward, in place in Bf
      if (active) {
        float s1 = 0.f, s2 = 0.f;
        for (int i = 0; i < h; ++i) {
          const float dx = br[i] * p[of.g2 + i];
          s1 += dx;
          s2 = fmaf(dx, ar[i], s2);
        }
        s1 *= invh, s2 *= invh;
        for (int i = 0; i < h; ++i) br[i] = rstd2 * (br[i] * p[of.g2 + i] - s1 - ar[i] * s2);
      }
      __syncthreads();
      // ---- d W1, d b1
      for (int e = tid; e < C * h; e += NX_THREADS) {
        const int c = e / h, o = e - c * h;
        const float g = p[of.g1 + c], b = p[of.be1 + c];
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s = fmaf(nx_relu(fmaf(g, X[r * LX + c], b)), Bf[r * LH + o], s);
        nx_acc(gp + of.W1 + e, first, s);
      }
      for (int o = tid; o < h; o += NX_THREADS) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += Bf[r * LH + o];
        nx_acc(gp + of.b1 + o, first, s);
      }
      // ---- d u1 = gate1 (d z1 . W1^T); d gamma1 / d beta1 over the wave; G += LN1 backward (every thread walks the
      // loop: the wave reductions need all 64 lanes, an idle thread adds zeros)
      {
        float s1 = 0.f, s2 = 0.f;
        for (int c = 0; c < C; c += 4) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          if (active) nx_dot4(br, p + of.W1 + c * h, h, h, acc);
          const float da[4] = {acc.x, acc.y, acc.z, acc.w};
          for (int q = 0; q < 4; ++q) {
            const float g = p[of.g1 + c + q];
            const float xh = xr[c + q];
            const float du = (active && fmaf(g, xh, p[of.be1 + c + q]) > 0.f) ? da[q] : 0.f;
            const float wg = wave_sum(du * xh), wb = wave_sum(du);
            if (lane == 0) red[wave * 2 * C + c + q] = wg, red[wave * 2 * C + C + c + q] = wb;
            const float dx = du * g;
            s1 += dx;
            s2 = fmaf(dx, xh, s2);
            if (active) gr[c + q] = fmaf(rstd1, dx, gr[c + q]);
          }
        }
        s1 *= invC, s2 *= invC;
        if (active)
          for (int c = 0; c < C; ++c) gr[c] -= rstd1 * fmaf(xr[c], s2, s1);
      }
      __syncthreads();
      for (int e = tid; e < 2 * C; e += NX_THREADS) {
        const float s = (red[e] + red[2 * C + e]) + (red[4 * C + e] + red[6 * C + e]);
        nx_acc(gp + (e < C ? of.g1 + e : of.be1 + e - C), first, s);
      }
    }
    __syncthreads();
    float* __restrict__ dst = dhist + base * T * C;
    for (int e = tid; e < rows * C; e += NX_THREADS) {
      const int r = e / C;
      dst[e] = G[r * LX + (e - r * C)];
    }
  }
}

// ids and labels of the training feed [Hn G, T] -> the (h, t, g) row order of model_output: out[(h T + t) G + g]
__global__ void __launch_bounds__(256) nx_rows_kernel(const int* __restrict__ items, const int* __restrict__ cates,
                                                      const float* __restrict__ labels, long n, int T, int G,
                                                      int* __restrict__ items_t, int* __restrict__ cates_t,
                                                      float* __restrict__ labels_t) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long ht = e / G;
  const int g = (int)(e - ht * G);
  const long hh = ht / T;
  const int t = (int)(ht - hh * T);
  const long s = (hh * G + g) * T + t;
  items_t[e] = items[s];
  cates_t[e] = cates[s];
  labels_t[e] = labels[s];
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int clsr_nextitnet_rows(const int* items, const int* cates, const float* labels, long Hn, int T, int G,
                                   int* items_t, int* cates_t, float* labels_t, void* stream) {
  CLSR_CHECK_ARG(items && cates && labels && items_t && cates_t && labels_t);
  CLSR_CHECK_ARG(Hn > 0 && T > 0 && G > 0 && Hn * T * G < (1L << 31));
  const long n = Hn * T * G;
  hipLaunchKernelGGL(nx_rows_kernel, dim3(clsr_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, items, cates, labels,
                     n, T, G, items_t, cates_t, labels_t);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_nextitnet_fwd(const float* hist, long Hn, int T, int C, const float* params, int k, int nblocks,
                                  const int* dilations, float* saved, float* out, int ldo, int rep, int last_only,
                                  void* stream) {
  CLSR_CHECK_ARG(hist && params && dilations && out);
  CLSR_CHECK_ARG(Hn > 0 && rep >= 1 && ldo >= C);
  CLSR_CHECK_SUPPORTED(clsr_nextitnet_supported(T, C, k, nblocks, 1));
  CLSR_CHECK_SUPPORTED(Hn * T * rep < (1L << 31) / NX_MAX_C);
  const int S = nx_slice(T, C, 0);
  const size_t shmem = (size_t)S * nx_fwd_hist_floats(T, C) * sizeof(float);       // <= 64 KB by nx_slice
  long grid = (Hn + S - 1) / S;
  if (grid > 2 * NX_MAX_PARTS) grid = 2 * NX_MAX_PARTS;
  hipLaunchKernelGGL(nx_fwd_kernel, dim3((unsigned)grid), dim3(NX_THREADS), shmem, (hipStream_t)stream, hist, Hn, T, C,
                     params, k, nblocks, dilations, saved, out, ldo, rep, last_only, S);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_nextitnet_bwd(const float* dout, const float* saved, long Hn, int T, int C, const float* params,
                                  int k, int nblocks, const int* dilations, float* dhist, float* partial,
                                  void* stream) {
  CLSR_CHECK_ARG(dout && saved && params && dilations && dhist && partial);
  CLSR_CHECK_ARG(Hn > 0);
  CLSR_CHECK_SUPPORTED(clsr_nextitnet_supported(T, C, k, nblocks, 1));
  CLSR_CHECK_SUPPORTED(Hn * T < (1L << 31) / NX_MAX_C);
  const int S = nx_slice(T, C, 1);
  const size_t shmem = (size_t)(S * nx_bwd_hist_floats(T, C) + nx_bwd_fixed_floats(C)) * sizeof(float);
  const int parts = clsr_nextitnet_parts(Hn, T, C, k, nblocks);
  hipLaunchKernelGGL(nx_bwd_kernel, dim3((unsigned)parts), dim3(NX_THREADS), shmem, (hipStream_t)stream, dout, saved, Hn,
                     T, C, params, k, nblocks, dilations, dhist, partial, S);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}
