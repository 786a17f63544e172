// NCF (models/sequential/ncf.py): the whole graph between the ids and the logit, per feed line l with user u(l), item i(l):
//
//   gmf[l]   = user_gmf[u] * item_gmf[i]                                                       [Du]
//   a_0[l]   = user_mlp[u] ++ item_mlp[i]                                                      [2 Du]
//   a_j[l]   = relu(b_j + a_{j-1}[l] . W_j)        j = 1 .. nl, W_j [n_{j-1}, n_j], n_0 = 2 Du
//   logit[l] = (gmf[l] ++ a_nl[l]) . w_out                                                     w_out [Du + n_nl]
//
// Parameter block (floats, the order the reference creates the variables in, each tensor contiguous, no padding: every
// width is a multiple of 4):   W_1 | b_1 | ... | W_nl | b_nl | w_out      -- the gradient block has the same layout.
//
// One pass over the lines: the parameter block sits in LDS for the whole launch (W_j with a row stride of n_j + 1 words,
// so that the transposed reads of the backward pass hit distinct banks), a workgroup of 256 threads walks tiles of
// NCF_TL / G * G lines -- whole softmax groups -- whose activations live in LDS beside it: gmf | a_0 | a_1 .. a_nl per
// line.  The backward pass of a tile overwrites a_j with dz_j in place, so a tile costs 3 Du + sum n_j (+ 1) words a line.
// Arithmetic: plain fp32 FMA chains (four interleaved chains per sum, the bias in the first); the fp32-input MFMAs of this chip run at the vector FMA
// rate and the products are small (ncf.yaml: 9 680 multiply-adds a line).
// No atomics: every output element has one owner thread.  A workgroup sums the dense gradients of its tiles, tile after
// tile, into its own row of the partial buffer (the first tile stores); the rows are reduced in a fixed order by the
// caller's partial-sum reduction.  Loss and the squared norms of the four slice sets are per-workgroup doubles that the
// second launch adds up in ascending workgroup order.
#include "common.h"

#define NCF_TL 16             // lines per tile (at most), so the largest softmax group
#define NCF_MAXW 128          // largest Du / tower width
#define NCF_MAXL 4            // tower layers
#define NCF_LDS_FLOATS 16320  // 64 KB less the 256 bytes kept for the block reductions
#define NCF_MAX_PARTS 256      // one workgroup a compute unit
#define NCF_STATS 5           // loss | sum of squares of d user_gmf, d user_mlp, d item_gmf, d item_mlp

struct NcfShape { int Du, nl, w[NCF_MAXL]; };

static NcfShape ncf_shape(int Du, int nl, int w0, int w1, int w2, int w3) {
  NcfShape s = {Du, nl, {w0, w1, w2, w3}};
  return s;
}
static bool ncf_dims_ok(const NcfShape& s) {
  if (s.Du <= 0 || s.Du % 4 || s.Du > NCF_MAXW || s.nl < 1 || s.nl > NCF_MAXL) return false;
  for (int j = 0; j < s.nl; ++j)
    if (s.w[j] <= 0 || s.w[j] % 4 || s.w[j] > NCF_MAXW) return false;
  return true;
}
static long ncf_param_floats(const NcfShape& s) {
  long n = 0;
  int K = 2 * s.Du;
  for (int j = 0; j < s.nl; ++j) { n += (long)K * s.w[j] + s.w[j]; K = s.w[j]; }
  return n + s.Du + K;
}
__host__ __device__ static inline int ncf_line_stride(const NcfShape& s) {
  int n = 3 * s.Du + 1;
  for (int j = 0; j < s.nl; ++j) n += s.w[j];
  return n;
}
static long ncf_lds_floats(const NcfShape& s) {
  long n = 0;
  int K = 2 * s.Du;
  for (int j = 0; j < s.nl; ++j) { n += (long)K * (s.w[j] + 1) + s.w[j]; K = s.w[j]; }
  return n + s.Du + K + (long)NCF_TL * ncf_line_stride(s) + 2 * NCF_TL;
}

extern "C" int clsr_ncf_max_width(void) { return NCF_MAXW; }
extern "C" int clsr_ncf_max_layers(void) { return NCF_MAXL; }
extern "C" int clsr_ncf_max_group(void) { return NCF_TL; }
extern "C" long clsr_ncf_lds_budget_floats(void) { return NCF_LDS_FLOATS; }
extern "C" long clsr_ncf_lds_floats(int Du, int nl, int w0, int w1, int w2, int w3) {
  const NcfShape s = ncf_shape(Du, nl, w0, w1, w2, w3);
  return ncf_dims_ok(s) ? ncf_lds_floats(s) : 0;
}
// G: lines of a softmax group (1: scoring)
extern "C" int clsr_ncf_supported(int Du, int nl, int w0, int w1, int w2, int w3, int G) {
  const NcfShape s = ncf_shape(Du, nl, w0, w1, w2, w3);
  return ncf_dims_ok(s) && G >= 1 && G <= NCF_TL && ncf_lds_floats(s) <= NCF_LDS_FLOATS;
}
extern "C" long clsr_ncf_param_floats(int Du, int nl, int w0, int w1, int w2, int w3) {
  const NcfShape s = ncf_shape(Du, nl, w0, w1, w2, w3);
  return ncf_dims_ok(s) ? ncf_param_floats(s) : 0;
}
extern "C" int clsr_ncf_tile_lines(int G) { return G >= 1 && G <= NCF_TL ? NCF_TL / G * G : 0; }
extern "C" int clsr_ncf_parts(long B, int G) {
  const int lt = clsr_ncf_tile_lines(G);
  if (B <= 0 || !lt) return 0;
  const long tiles = (B + lt - 1) / lt;
  return (int)(tiles < NCF_MAX_PARTS ? tiles : NCF_MAX_PARTS);
}
// [parts][NCF_STATS] doubles, then [parts][param floats]
extern "C" long clsr_ncf_workspace_floats(long B, int G, int Du, int nl, int w0, int w1, int w2, int w3) {
  const long P = clsr_ncf_param_floats(Du, nl, w0, w1, w2, w3);
  const int parts = clsr_ncf_parts(B, G);
  return parts && P ? (long)parts * (2 * NCF_STATS + P) : 0;
}

struct NcfArgs {
  const int* users; const int* items; const float* labels;
  const float* ug; const float* um; const float* ig; const float* im;
  const float* params;
  float* logit; float* mo; float* dlogit;
  float* d_ug; float* d_um; float* d_ig; float* d_im;
  int* uid_out; float* part; double* stats;
  long B; int udiv; int LT; int G; float scale;
  NcfShape s;
};

template <bool TRAIN>
__global__ void __launch_bounds__(256) ncf_kernel(NcfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ double red[NCF_STATS][4];
  const int tid = threadIdx.x;
  const NcfShape s = a.s;
  const int Du = s.Du, nl = s.nl, K0 = 2 * Du;
  // ---- LDS and parameter-block offsets of every layer
  int wl[NCF_MAXL], bl[NCF_MAXL], wg[NCF_MAXL], ao[NCF_MAXL + 1];
  int lo = 0, go = 0, act = Du, K = K0, aoL = 0;
  ao[0] = act; act += K0;                    // line: gmf @0 | a_0 @Du | a_1 | ...
#pragma unroll
  for (int j = 0; j < NCF_MAXL; ++j) {
    if (j < nl) {
      wl[j] = lo; lo += K * (s.w[j] + 1);
      bl[j] = lo; lo += s.w[j];
      wg[j] = go; go += K * s.w[j] + s.w[j];
      ao[j + 1] = act; aoL = act; act += s.w[j];
      K = s.w[j];
    } else { wl[j] = bl[j] = wg[j] = 0; ao[j + 1] = 0; }
  }
  const int last = K, WO = Du + last;        // K: width of the last layer
  const int wol = lo, wog = go;              // w_out
  lo += WO;
  const int S = ncf_line_stride(s);
  float* tile = lds + lo;
  float* lg = tile + NCF_TL * S;             // logit | dlogit of the tile's lines
  float* dlg = lg + NCF_TL;
  // ---- parameters -> LDS
  K = K0;
#pragma unroll
  for (int j = 0; j < NCF_MAXL; ++j) {
    if (j >= nl) break;
    const int n = s.w[j];
    for (int e = tid; e < K * n; e += 256) {
      const int k = e / n, c = e - k * n;
      lds[wl[j] + k * (n + 1) + c] = a.params[wg[j] + e];
    }
    for (int e = tid; e < n; e += 256) lds[bl[j] + e] = a.params[wg[j] + K * n + e];
    K = n;
  }
  for (int e = tid; e < WO; e += 256) lds[wol + e] = a.params[wog + e];
  double loss = 0.0, ssq[4] = {0.0, 0.0, 0.0, 0.0};
  const long ntiles = (a.B + a.LT - 1) / a.LT;
  float* part = TRAIN ? a.part + (long)blockIdx.x * (wog + WO) : nullptr;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool first = t == blockIdx.x;
    const long l0 = t * a.LT;
    const int nt = (int)(a.B - l0 < a.LT ? a.B - l0 : a.LT);
    __syncthreads();
    // ---- the four row gathers
    const int D4 = Du >> 2;
    for (int e = tid; e < nt * D4; e += 256) {
      const int l = e / D4, c = (e - l * D4) * 4;
      const long u = a.users[(l0 + l) / a.udiv], i = a.items[l0 + l];
      const f32x4 vug = ld4(a.ug + u * Du + c), vig = ld4(a.ig + i * Du + c);
      const f32x4 vum = ld4(a.um + u * Du + c), vim = ld4(a.im + i * Du + c);
      float* ln = tile + l * S;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ln[c + q] = vug[q] * vig[q];
        ln[Du + c + q] = vum[q];
        ln[2 * Du + c + q] = vim[q];
      }
      if (TRAIN && c == 0) a.uid_out[l0 + l] = (int)u;
    }
    __syncthreads();
    // ---- tower
    K = K0;
#pragma unroll
    for (int j = 0; j < NCF_MAXL; ++j) {
      if (j >= nl) break;
      const int n = s.w[j];
      const float* W = lds + wl[j];
      for (int e = tid; e < nt * n; e += 256) {
        const int l = e / n, c = e - l * n;
        const float* x = tile + l * S + ao[j];
        // four independent chains over k (K is a multiple of 4): the LDS reads of a step are in flight together
        const float* w = W + c;
        const int n1 = n + 1;
        float a0 = lds[bl[j] + c], a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int k = 0; k < K; k += 4) {
          a0 = fmaf(x[k], w[k * n1], a0);
          a1 = fmaf(x[k + 1], w[(k + 1) * n1], a1);
          a2 = fmaf(x[k + 2], w[(k + 2) * n1], a2);
          a3 = fmaf(x[k + 3], w[(k + 3) * n1], a3);
        }
        tile[l * S + ao[j + 1] + c] = fmaxf((a0 + a1) + (a2 + a3), 0.f);
      }
      __syncthreads();
      K = n;
    }
    // ---- logit: 16 lanes a line, lane q sums the columns q, q + 16, ...; model_output = gmf ++ a_nl
    {
      const int l = tid >> 4, q = tid & 15;
      float acc = 0.f;
      if (l < nt) {
        const float* ln = tile + l * S;
        for (int c = q; c < WO; c += 16) {
          const float v = c < Du ? ln[c] : ln[aoL + c - Du];
          acc = fmaf(v, lds[wol + c], acc);
          if (a.mo) a.mo[(l0 + l) * WO + c] = v;
        }
      }
      acc = row16_sum(acc);
      if (l < nt && q == 0) { lg[l] = acc; a.logit[l0 + l] = acc; }
    }
    if (!TRAIN) continue;
    __syncthreads();
    // ---- group softmax (csrc/heads.hip: softmax_loss_kernel), one thread a group
    if (tid < nt / a.G) {
      const int G = a.G;
      const float* x = lg + tid * G;
      const float* lb = a.labels + l0 + tid * G;
      float mx = -INFINITY;
      for (int g = 0; g < G; ++g) mx = fmaxf(mx, x[g]);
      float sum = 0.f;
      for (int g = 0; g < G; ++g) sum += __expf(x[g] - mx);
      const float lse = mx + __logf(sum);
      int npos = 0;
      float local = 0.f;
      for (int g = 0; g < G; ++g)
        if (lb[g] == 1.0f) { ++npos; local -= (x[g] - lse); }
      for (int g = 0; g < G; ++g) {
        const float d = a.scale * ((float)npos * __expf(x[g] - lse) - (lb[g] == 1.0f ? 1.0f : 0.0f));
        dlg[tid * G + g] = d;
        if (a.dlogit) a.dlogit[l0 + tid * G + g] = d;
      }
      loss += (double)local;
    }
    __syncthreads();
    // ---- d w_out; the slices of the two GMF tables
    for (int c = tid; c < WO; c += 256) {
      float acc = 0.f;
      for (int l = 0; l < nt; ++l) acc = fmaf(dlg[l], c < Du ? tile[l * S + c] : tile[l * S + aoL + c - Du], acc);
      part[wog + c] = first ? acc : part[wog + c] + acc;
    }
    for (int e = tid; e < nt * D4; e += 256) {
      const int l = e / D4, c = (e - l * D4) * 4;
      const long u = a.users[(l0 + l) / a.udiv], i = a.items[l0 + l];
      const f32x4 vug = ld4(a.ug + u * Du + c), vig = ld4(a.ig + i * Du + c);
      const float d = dlg[l];
      f32x4 du, di;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float dg = d * lds[wol + c + q];
        du[q] = dg * vig[q];
        di[q] = dg * vug[q];
        ssq[0] += (double)du[q] * du[q];
        ssq[2] += (double)di[q] * di[q];
      }
      st4(a.d_ug + (l0 + l) * Du + c, du);
      st4(a.d_ig + (l0 + l) * Du + c, di);
    }
    __syncthreads();
    // ---- dz_nl over a_nl, in place
    for (int e = tid; e < nt * last; e += 256) {
      const int l = e / last, c = e - l * last;
      float* p = tile + l * S + aoL + c;
      *p = *p > 0.f ? dlg[l] * lds[wol + Du + c] : 0.f;
    }
    __syncthreads();
    // ---- tower backward, last layer first
#pragma unroll
    for (int j = NCF_MAXL - 1; j >= 0; --j) {
      if (j >= nl) continue;
      const int n = s.w[j], Kj = j ? s.w[j - 1] : K0;
      const float* W = lds + wl[j];
      // d W_j | d b_j from the layer's input and dz_j
      for (int e = tid; e < Kj * n + n; e += 256) {
        float acc = 0.f;
        if (e < Kj * n) {
          const int k = e / n, c = e - k * n;
          const float* xi = tile + ao[j] + k;
          const float* dz = tile + ao[j + 1] + c;
          float b0 = 0.f, b1 = 0.f;
          int l = 0;
          for (; l + 1 < nt; l += 2) {
            b0 = fmaf(xi[l * S], dz[l * S], b0);
            b1 = fmaf(xi[(l + 1) * S], dz[(l + 1) * S], b1);
          }
          if (l < nt) b0 = fmaf(xi[l * S], dz[l * S], b0);
          acc = b0 + b1;
        } else {
          const int c = e - Kj * n;
          for (int l = 0; l < nt; ++l) acc += tile[l * S + ao[j + 1] + c];
        }
        part[wg[j] + e] = first ? acc : part[wg[j] + e] + acc;
      }
      __syncthreads();
      // d a_{j-1} = dz_j . W_j^T, gated into dz_{j-1} over a_{j-1} (j = 0: the slices of the two MLP tables)
      for (int e = tid; e < nt * Kj; e += 256) {
        const int l = e / Kj, k = e - l * Kj;
        const float* dz = tile + l * S + ao[j + 1];
        const float* w = W + k * (n + 1);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;      // (n is a multiple of 4)
        for (int c = 0; c < n; c += 4) {
          a0 = fmaf(dz[c], w[c], a0);
          a1 = fmaf(dz[c + 1], w[c + 1], a1);
          a2 = fmaf(dz[c + 2], w[c + 2], a2);
          a3 = fmaf(dz[c + 3], w[c + 3], a3);
        }
        const float acc = (a0 + a1) + (a2 + a3);
        if (j) {
          float* p = tile + l * S + ao[j] + k;
          *p = *p > 0.f ? acc : 0.f;
        } else if (k < Du) {
          a.d_um[(l0 + l) * Du + k] = acc;
          ssq[1] += (double)acc * acc;
        } else {
          a.d_im[(l0 + l) * Du + k - Du] = acc;
          ssq[3] += (double)acc * acc;
        }
      }
      __syncthreads();
    }
  }
  if (TRAIN) {
    const double v0 = block256_sum_d(loss, red[0]);
    const double v1 = block256_sum_d(ssq[0], red[1]), v2 = block256_sum_d(ssq[1], red[2]);
    const double v3 = block256_sum_d(ssq[2], red[3]), v4 = block256_sum_d(ssq[3], red[4]);
    if (tid == 0) {
      double* st = a.stats + (long)blockIdx.x * NCF_STATS;
      st[0] = v0; st[1] = v1; st[2] = v2; st[3] = v3; st[4] = v4;
    }
  }
}

// loss_out[0] += scale * sum of the workgroups' losses; sumsq4[q] = sum of their squared slice norms: ascending order
__global__ void ncf_finish_kernel(const double* __restrict__ stats, int parts, double scale, double* __restrict__ loss_out,
                                  double* __restrict__ sumsq4) {
  const int q = threadIdx.x;
  if (q >= NCF_STATS) return;
  double s = 0.0;
  for (int p = 0; p < parts; ++p) s += stats[(long)p * NCF_STATS + q];
  if (q == 0) loss_out[0] += s * scale;
  else if (sumsq4) sumsq4[q - 1] = s;
}

#define NCF_CHECK_SHAPE()                                                                                    \
  const NcfShape sh = ncf_shape(Du, nl, w0, w1, w2, w3);                                                      \
  CLSR_CHECK_ARG(users && items && user_gmf && user_mlp && item_gmf && item_mlp && params && logit);          \
  CLSR_CHECK_ARG(B > 0 && B < (1L << 31) && user_div >= 1);                                                   \
  CLSR_CHECK_ARG(ncf_dims_ok(sh));                                                                            \
  CLSR_CHECK_ARG(ncf_lds_floats(sh) <= NCF_LDS_FLOATS)

static void ncf_fill(NcfArgs& a, const int* users, int user_div, const int* items, const float* ug, const float* um,
                     const float* ig, const float* im, const float* params, const NcfShape& sh, long B, float* logit,
                     float* mo) {
  a.users = users; a.udiv = user_div; a.items = items; a.ug = ug; a.um = um; a.ig = ig; a.im = im; a.params = params;
  a.s = sh; a.B = B; a.logit = logit; a.mo = mo;
}

extern "C" int clsr_ncf_score(const int* users, int user_div, const int* items, const float* user_gmf,
                              const float* user_mlp, const float* item_gmf, const float* item_mlp, const float* params,
                              int Du, int nl, int w0, int w1, int w2, int w3, long B, float* logit, float* model_output,
                              void* stream) {
  NCF_CHECK_SHAPE();
  NcfArgs a = {};
  ncf_fill(a, users, user_div, items, user_gmf, user_mlp, item_gmf, item_mlp, params, sh, B, logit, model_output);
  a.LT = NCF_TL; a.G = 1;
  const long tiles = (B + NCF_TL - 1) / NCF_TL;
  const unsigned grid = (unsigned)(tiles < 1024 ? tiles : 1024);
  hipLaunchKernelGGL(ncf_kernel<false>, dim3(grid), dim3(256), (size_t)ncf_lds_floats(sh) * sizeof(float),
                     (hipStream_t)stream, a);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_ncf_train(const int* users, int user_div, const int* items, const float* labels,
                              const float* user_gmf, const float* user_mlp, const float* item_gmf,
                              const float* item_mlp, const float* params, int Du, int nl, int w0, int w1, int w2, int w3,
                              long B, int G, float scale, float* logit, float* model_output, float* dlogit,
                              float* d_user_gmf, float* d_user_mlp, float* d_item_gmf, float* d_item_mlp, int* user_ids,
                              float* workspace, double* loss_out, double* sumsq4, void* stream) {
  NCF_CHECK_SHAPE();
  CLSR_CHECK_ARG(labels && d_user_gmf && d_user_mlp && d_item_gmf && d_item_mlp && user_ids && workspace && loss_out);
  CLSR_CHECK_ARG(G >= 1 && G <= NCF_TL && B % G == 0 && ((uintptr_t)workspace & 7) == 0);
  NcfArgs a = {};
  ncf_fill(a, users, user_div, items, user_gmf, user_mlp, item_gmf, item_mlp, params, sh, B, logit, model_output);
  const int parts = clsr_ncf_parts(B, G);
  a.labels = labels; a.dlogit = dlogit; a.d_ug = d_user_gmf; a.d_um = d_user_mlp; a.d_ig = d_item_gmf; a.d_im = d_item_mlp;
  a.uid_out = user_ids; a.stats = (double*)workspace; a.part = workspace + 2L * NCF_STATS * parts;
  a.LT = clsr_ncf_tile_lines(G); a.G = G; a.scale = scale;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ncf_kernel<true>, dim3(parts), dim3(256), (size_t)ncf_lds_floats(sh) * sizeof(float), s, a);
  CLSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(ncf_finish_kernel, dim3(1), dim3(64), 0, s, a.stats, parts, (double)scale, loss_out, sumsq4);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}
