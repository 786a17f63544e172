// The other optimisers of the reference (base_model.py:249-279) for the CLSR step (gfx950): GradientDescent (sgd, gd),
// ProximalGradientDescent (pgd, l1 = l2 = 0), Adagrad, ProximalAdagrad (padagrad, l1 = l2 = 0), RMSProp, Adadelta and
// Ftrl, each with the TF 1.15 defaults the reference leaves in place (it passes only the learning rate):
//
//   sgd / gd / pgd  var -= lr*g
//   adagrad         acc += g^2; var -= lr*g*rsqrt(acc)                                  acc  <- 0.1
//   padagrad        acc += g^2; var = var - g*(lr*rsqrt(acc))       (the proximal order)  acc  <- 0.1
//   rmsprop         ms += (g^2 - ms)*(1 - 0.9); mom = 0*mom + lr*g*rsqrt(ms + 1e-10); var -= mom     ms <- 1, mom <- 0
//   adadelta        acc = 0.95 acc + 0.05 g^2; u = sqrt(accu + 1e-8)*rsqrt(acc + 1e-8)*g; var -= lr*u;
//                   accu = 0.95 accu + 0.05 u^2                                                       acc, accu <- 0
//   ftrl            n = acc + g^2; lin += g - (sqrt(n) - sqrt(acc))/lr*var; var = |lin| > 0 ? -lin/(sqrt(n)/lr) : 0;
//                   acc = n  (lr_power -0.5, l1 = l2 = l2_shrinkage = 0)                               acc <- 0.1, lin <- 0
//
// g is the gradient after the per-variable tf.clip_by_norm (same clip factor as the Adam kernels of optim.hip).  The
// embedding tables follow TF's sparse_apply_* ops: ONLY the touched rows (flag map / involved-row list) are read and
// written; the other rows keep their values and slots bit for bit.  The optimiser is a template parameter: an
// instantiation loads and stores its own slots only (bytes per element: sgd 16, adagrad 24, the two-slot ones 32).
// Every kernel returns without touching anything while state[4] (the abort flag of the step) is raised.
#include <stdlib.h>
#include "tableopt.h"
#include "clsr_hip.h"

enum { TF_SGD = 0, TF_ADAGRAD = 1, TF_PADAGRAD = 2, TF_RMSPROP = 3, TF_ADADELTA = 4, TF_FTRL = 5, TF_NOPT = 6 };

__host__ __device__ constexpr int tf_slots(int o) {
  return o == TF_SGD ? 0 : (o == TF_ADAGRAD || o == TF_PADAGRAD) ? 1 : 2;
}

extern "C" int clsr_tf_opt_slots(int opt) { return opt >= 0 && opt < TF_NOPT ? tf_slots(opt) : CLSR_EINVAL; }

// one element: g already clipped; p, s1, s2 updated in place (s1 / s2 unused by the optimisers that lack them)
template <int O>
__device__ __forceinline__ void tf_update(float g, float lr, float& p, float& s1, float& s2) {
  if (O == TF_SGD) {
    p -= lr * g;
  } else if (O == TF_ADAGRAD) {
    s1 += g * g;
    p -= lr * g * (1.0f / sqrtf(s1));
  } else if (O == TF_PADAGRAD) {
    s1 += g * g;
    p = p - g * (lr * (1.0f / sqrtf(s1)));
  } else if (O == TF_RMSPROP) {
    const float rho = 0.9f, eps = 1e-10f;
    s1 += (g * g - s1) * (1.0f - rho);
    s2 = 0.0f * s2 + lr * g * (1.0f / sqrtf(s1 + eps));
    p -= s2;
  } else if (O == TF_ADADELTA) {
    const float rho = 0.95f, eps = 1e-8f;
    s1 = rho * s1 + (1.0f - rho) * g * g;
    const float u = sqrtf(s2 + eps) * (1.0f / sqrtf(s1 + eps)) * g;
    p -= lr * u;
    s2 = rho * s2 + (1.0f - rho) * u * u;
  } else {   // TF_FTRL
    const float n = s1 + g * g;
    const float sn = sqrtf(n);
    s2 += g - (sn - sqrtf(s1)) / lr * p;
    p = fabsf(s2) > 0.f ? -s2 / (sn / lr) : 0.f;
    s1 = n;
  }
}

// ---------------------------------------------------------------------------- flat dense update
// One element per thread-iteration (the dense block is ~0.1-1 M values); skip[tensor] != 0: a variable the reference
// graph gives no gradient (apply_gradients skips it) -- its value and slots stay, its gradient buffer is cleared.
template <int O>
__global__ void __launch_bounds__(256) dense_tf_kernel(float* __restrict__ param, float* __restrict__ grad,
                                                       float* __restrict__ s1, float* __restrict__ s2,
                                                       const int* __restrict__ seg_of,
                                                       const unsigned char* __restrict__ skip,
                                                       const double* __restrict__ sumsq, float clip_norm,
                                                       const double* __restrict__ state, float lr, int n) {
  if (state[4] != 0.0) return;      // the step was aborted (a collective / grid barrier gave up): touch nothing
  constexpr int NS = tf_slots(O);
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const int seg = seg_of[e];
    if (!(skip && skip[seg])) {
      const float g = grad[e] * clip_factor(sumsq[seg], clip_norm);
      float p = param[e], a = NS > 0 ? s1[e] : 0.f, b = NS > 1 ? s2[e] : 0.f;
      tf_update<O>(g, lr, p, a, b);
      param[e] = p;
      if (NS > 0) s1[e] = a;
      if (NS > 1) s2[e] = b;
    }
    grad[e] = 0.f;
  }
}

template <template <int> class K, typename... A>
static void launch_opt(int opt, dim3 grid, hipStream_t s, A... args) {
  switch (opt) {
    case TF_SGD: hipLaunchKernelGGL(K<TF_SGD>::fn, grid, dim3(256), 0, s, args...); break;
    case TF_ADAGRAD: hipLaunchKernelGGL(K<TF_ADAGRAD>::fn, grid, dim3(256), 0, s, args...); break;
    case TF_PADAGRAD: hipLaunchKernelGGL(K<TF_PADAGRAD>::fn, grid, dim3(256), 0, s, args...); break;
    case TF_RMSPROP: hipLaunchKernelGGL(K<TF_RMSPROP>::fn, grid, dim3(256), 0, s, args...); break;
    case TF_ADADELTA: hipLaunchKernelGGL(K<TF_ADADELTA>::fn, grid, dim3(256), 0, s, args...); break;
    default: hipLaunchKernelGGL(K<TF_FTRL>::fn, grid, dim3(256), 0, s, args...); break;
  }
}

template <int O> struct DenseK { static constexpr auto fn = dense_tf_kernel<O>; };

static int check_slots(int opt, const void* s1, const void* s2) {
  CLSR_CHECK_ARG(opt >= 0 && opt < TF_NOPT);
  CLSR_CHECK_ARG(tf_slots(opt) < 1 || s1);
  CLSR_CHECK_ARG(tf_slots(opt) < 2 || s2);
  return CLSR_OK;
}

extern "C" int clsr_dense_tf(int opt, float* param, float* grad, float* s1, float* s2, const int* seg_of,
                             const unsigned char* skip, const double* sumsq, float clip_norm, const double* state,
                             float lr, int n, void* stream) {
  CLSR_CHECK_ARG(param && grad && seg_of && sumsq && state && n > 0 && lr > 0.f);
  int rc = check_slots(opt, s1, s2);
  if (rc) return rc;
  int blocks = clsr_cdiv(n, 256);
  if (blocks > 2048) blocks = 2048;
  launch_opt<DenseK>(opt, dim3(blocks), (hipStream_t)stream, param, grad, s1, s2, seg_of, skip, sumsq, clip_norm, state,
                     lr, n);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---------------------------------------------------------------------------- multi-table flag sweep
// blockIdx.y = table; desc.m / desc.v are slot 1 / slot 2 (NULL when the optimiser has fewer).  Flagged rows only.
struct TfTablesArgs {
  clsr_table_desc t[4];
  float clip_norm;
  float lr;
  const double* state;
  int clear_flags;       // the v4 sweep clears the flags itself (every chunk of a row lies in one wave)
};

template <int O>
__global__ void __launch_bounds__(256) tables_tf_multi_kernel(TfTablesArgs a) {
  const clsr_table_desc d = a.t[blockIdx.y];
  const float factor = clip_factor(d.sumsq_adam, d.sumsq_stride, d.nsum, a.clip_norm);
  if (a.state[4] != 0.0) return;    // aborted step: touch nothing
  constexpr int NS = tf_slots(O);
  const long total = d.V * d.C;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    if (!d.flags[e / d.C]) continue;
    float p = d.table[e], s1 = NS > 0 ? d.m[e] : 0.f, s2 = NS > 1 ? d.v[e] : 0.f;
    tf_update<O>(d.grad[e] * factor, a.lr, p, s1, s2);
    d.table[e] = p;
    if (NS > 0) d.m[e] = s1;
    if (NS > 1) d.v[e] = s2;
    d.grad[e] = 0.f;
  }
}

// Rows of 4 k values, 16-byte aligned operands: one 16-byte access per operand and lane, the loads of two grid strides
// issued together from clamped addresses and selected by the row flags afterwards (as adam_sweep_v4 of tableopt.h).
// No LDS: this launch runs beside the fused encoder tail (csrc/encbwd.hip), which owns every CU's LDS.
// When the chunks of a row count divides 64 (a.clear_flags), all chunks of a row lie in ONE wave and the same unroll
// slot -- the flag is read by one load instruction of that wave before the row's first lane clears it: the flags are
// cleared in this launch, race-free.
template <int O>
__global__ void __launch_bounds__(256) tables_tf_multi_v4_kernel(TfTablesArgs a) {
  __builtin_amdgcn_s_setprio(3);
  const clsr_table_desc d = a.t[blockIdx.y];
  const float factor = clip_factor(d.sumsq_adam, d.sumsq_stride, d.nsum, a.clip_norm);
  if (a.state[4] != 0.0) return;    // aborted step: touch nothing
  constexpr int NS = tf_slots(O);
  const unsigned QC = (unsigned)d.C >> 2, total = (unsigned)d.V * QC;
  const unsigned stride = gridDim.x * 256u;
  for (unsigned q0 = blockIdx.x * 256u + threadIdx.x; q0 < total; q0 += 2u * stride) {
    bool f[2];
    f32x4 g[2], w[2], m[2], v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned q = q0 + (unsigned)u * stride, qs = q < total ? q : 0u;
      f[u] = q < total && d.flags[qs / QC];
      g[u] = ld4(d.grad + 4L * qs);
      w[u] = ld4(d.table + 4L * qs);
      if (NS > 0) m[u] = ld4(d.m + 4L * qs);
      if (NS > 1) v[u] = ld4(d.v + 4L * qs);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!f[u]) continue;
      const unsigned q = q0 + (unsigned)u * stride;
      const long e = 4L * q;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float p = w[u][c], s1 = NS > 0 ? m[u][c] : 0.f, s2 = NS > 1 ? v[u][c] : 0.f;
        tf_update<O>(g[u][c] * factor, a.lr, p, s1, s2);
        w[u][c] = p;
        if (NS > 0) m[u][c] = s1;
        if (NS > 1) v[u][c] = s2;
      }
      st4(d.table + e, w[u]);
      if (NS > 0) st4(d.m + e, m[u]);
      if (NS > 1) st4(d.v + e, v[u]);
      st4(d.grad + e, f32x4{0.f, 0.f, 0.f, 0.f});
      if (a.clear_flags && q % QC == 0) d.flags[q / QC] = 0;
    }
  }
}

__global__ void __launch_bounds__(256) tables_tf_clear_flags_kernel(TfTablesArgs a) {
  if (a.state[4] != 0.0) return;
  const clsr_table_desc d = a.t[blockIdx.y];
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < d.V; e += (long)gridDim.x * blockDim.x) d.flags[e] = 0;
}

template <int O> struct TablesK { static constexpr auto fn = tables_tf_multi_kernel<O>; };
template <int O> struct TablesV4K { static constexpr auto fn = tables_tf_multi_v4_kernel<O>; };

extern "C" int clsr_tables_tf_multi(const clsr_table_desc* descs, int n, int opt, float clip_norm, const double* state,
                                    float lr, void* stream) {
  CLSR_CHECK_ARG(descs && n > 0 && n <= 4 && state && lr > 0.f);
  TfTablesArgs a = {};
  long mx = 1, mxv = 1;
  bool v4 = true, same_wave = true;
  for (int i = 0; i < n; ++i) {
    const clsr_table_desc& d = descs[i];
    CLSR_CHECK_ARG(d.table && d.grad && d.flags && d.sumsq_adam && d.nsum > 0 && d.V > 0 && d.C > 0);
    int rc = check_slots(opt, d.m, d.v);
    if (rc) return rc;
    a.t[i] = d;
    mx = d.V * d.C > mx ? d.V * d.C : mx;
    mxv = d.V > mxv ? d.V : mxv;
    if (d.C % 4 || d.V * d.C >= (1L << 31) ||
        (((uintptr_t)d.table | (uintptr_t)d.grad | (uintptr_t)d.m | (uintptr_t)d.v) & 15))
      v4 = false;
    if (64 % (d.C / 4 > 0 ? d.C / 4 : 1)) same_wave = false;
  }
  a.clip_norm = clip_norm; a.lr = lr; a.state = state;
  a.clear_flags = v4 && same_wave;
  hipStream_t s = (hipStream_t)stream;
  if (v4) {
    int blocks = clsr_cdiv(mx / 4, 256 * 2);
    if (blocks > 2048) blocks = 2048;
    launch_opt<TablesV4K>(opt, dim3(blocks, n), s, a);
  } else {
    int blocks = clsr_cdiv(mx, 256);
    if (blocks > 2048) blocks = 2048;
    launch_opt<TablesK>(opt, dim3(blocks, n), s, a);
  }
  CLSR_CHECK_LAUNCH();
  if (a.clear_flags) return CLSR_OK;
  int cb = clsr_cdiv(mxv, 256);
  if (cb > 512) cb = 512;
  hipLaunchKernelGGL(tables_tf_clear_flags_kernel, dim3(cb, n), dim3(256), 0, s, a);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---------------------------------------------------------------------------- row-list update (huge tables)
// ids / count from clsr_flags_compact (the involved rows); clears their gradient rows and flags.  VW = 4: 16-byte pieces
// (C % 4 == 0), VW = 1 otherwise; UN pieces per lane and trip, all their loads issued before the first one is used
// (random rows of a 38 GB table: the update is bound by the row reads in flight, as table_adam_rows_kernel).
template <int O, int VW, int UN>
__global__ void __launch_bounds__(256) table_tf_rows_kernel(
    float* __restrict__ table, float* __restrict__ grad_table, float* __restrict__ s1p, float* __restrict__ s2p,
    unsigned char* __restrict__ flags, const int* __restrict__ ids, const int* __restrict__ count, int C,
    const double* __restrict__ sumsq, int sumsq_stride, int nsum, float clip_norm, const double* __restrict__ state,
    float lr) {
  const float factor = clip_factor(sumsq, sumsq_stride, nsum, clip_norm);
  if (state[4] != 0.0) return;      // aborted step: touch nothing
  constexpr int NS = tf_slots(O);
  const int QC = C / VW;
  const long total = (long)count[0] * QC;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < total; i0 += stride * UN) {
    long e[UN], row[UN];
    int q[UN];
    bool ok[UN];
    float g[UN][VW], po[UN][VW], a[UN][VW], b[UN][VW];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const long i = i0 + u * stride;
      ok[u] = i < total;
      const long ic = ok[u] ? i : i0;
      const long r = ic / QC;
      q[u] = (int)(ic - r * QC);
      row[u] = ids[r];
      e[u] = row[u] * C + (long)q[u] * VW;
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (VW == 4) {
        *reinterpret_cast<f32x4*>(g[u]) = ld4(grad_table + e[u]);
        *reinterpret_cast<f32x4*>(po[u]) = ld4(table + e[u]);
        if (NS > 0) *reinterpret_cast<f32x4*>(a[u]) = ld4(s1p + e[u]);
        if (NS > 1) *reinterpret_cast<f32x4*>(b[u]) = ld4(s2p + e[u]);
      } else {
        g[u][0] = grad_table[e[u]];
        po[u][0] = table[e[u]];
        if (NS > 0) a[u][0] = s1p[e[u]];
        if (NS > 1) b[u][0] = s2p[e[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (!ok[u]) continue;
#pragma unroll
      for (int k = 0; k < VW; ++k) {
        float x = NS > 0 ? a[u][k] : 0.f, y = NS > 1 ? b[u][k] : 0.f;
        tf_update<O>(g[u][k] * factor, lr, po[u][k], x, y);
        a[u][k] = x;
        b[u][k] = y;
      }
      if (VW == 4) {
        st4(table + e[u], *reinterpret_cast<f32x4*>(po[u]));
        if (NS > 0) st4(s1p + e[u], *reinterpret_cast<f32x4*>(a[u]));
        if (NS > 1) st4(s2p + e[u], *reinterpret_cast<f32x4*>(b[u]));
        st4(grad_table + e[u], f32x4{0.f, 0.f, 0.f, 0.f});
      } else {
        table[e[u]] = po[u][0];
        if (NS > 0) s1p[e[u]] = a[u][0];
        if (NS > 1) s2p[e[u]] = b[u][0];
        grad_table[e[u]] = 0.f;
      }
      if (q[u] == 0) flags[row[u]] = 0;
    }
  }
}

template <int O> struct RowsV4K { static constexpr auto fn = table_tf_rows_kernel<O, 4, 2>; };
template <int O> struct RowsV1K { static constexpr auto fn = table_tf_rows_kernel<O, 1, 1>; };

extern "C" int clsr_table_tf_rows(int opt, float* table, float* grad_table, float* s1, float* s2, unsigned char* flags,
                                  const int* ids, const int* count, int cap, int C, const double* sumsq,
                                  int sumsq_stride, int nsum, float clip_norm, const double* state, float lr,
                                  void* stream) {
  CLSR_CHECK_ARG(table && grad_table && flags && ids && count && sumsq && state && cap > 0 && C > 0 && nsum > 0);
  CLSR_CHECK_ARG(lr > 0.f);
  int rc = check_slots(opt, s1, s2);
  if (rc) return rc;
  const bool vec = C % 4 == 0 &&
                   !(((uintptr_t)table | (uintptr_t)grad_table | (uintptr_t)s1 | (uintptr_t)s2) & 15);
  int blocks = clsr_cdiv((long)cap * C, 256 * 4 * (vec ? 2 : 1));
  if (blocks > 4096) blocks = 4096;
  if (vec)
    launch_opt<RowsV4K>(opt, dim3(blocks), (hipStream_t)stream, table, grad_table, s1, s2, flags, ids, count, C, sumsq,
                        sumsq_stride, nsum, clip_norm, state, lr);
  else
    launch_opt<RowsV1K>(opt, dim3(blocks), (hipStream_t)stream, table, grad_table, s1, s2, flags, ids, count, C, sumsq,
                        sumsq_stride, nsum, clip_norm, state, lr);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}
