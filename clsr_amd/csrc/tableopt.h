// The optimiser side of the embedding tables (csrc/optim.hip, csrc/multi.hip, csrc/optim_tf.hip), device only: the clip
// factor, ONE Adam element update, the three storage formats of a table as policies, and the loop skeletons of the Adam
// kernels (sweep, 16-byte sweep, involved-row list), each written once and instantiated per storage format.
#pragma once
#include "common.h"

// per-tensor tf.clip_by_norm: g * clip_norm / max(||g||, clip_norm)
__device__ __forceinline__ float clip_factor(double sumsq, float clip_norm) {
  if (clip_norm <= 0.f) return 1.0f;
  const float nrm = (float)sqrt(sumsq);
  return clip_norm / fmaxf(nrm, clip_norm);
}
// ... of a table: sumsq[i * stride], i < nsum, are the squared norms of its IndexedSlices pieces (lookup sites + involved rows)
__device__ __forceinline__ float clip_factor(const double* __restrict__ sumsq, int stride, int nsum, float clip_norm) {
  double tot = 0.0;
  for (int i = 0; i < nsum; ++i) tot += sumsq[(long)i * stride];
  return clip_factor(tot, clip_norm);
}

// The scalars of one table's Adam update
struct AdamStep {
  float factor, lr_t, b1, b2, eps;
};
// false: the step was aborted (a collective / grid barrier gave up -- csrc/p2p.hip, csrc/headsfused.hip): touch nothing
__device__ __forceinline__ bool adam_begin(AdamStep& s, const double* __restrict__ sumsq, int sumsq_stride, int nsum,
                                           float clip_norm, const double* __restrict__ adam_state, float b1, float b2,
                                           float eps) {
  s.factor = clip_factor(sumsq, sumsq_stride, nsum, clip_norm);
  if (adam_state[4] != 0.0) return false;
  s.lr_t = (float)adam_state[3];
  s.b1 = b1; s.b2 = b2; s.eps = eps;
  return true;
}

// One Adam element update (m, v, w in place; g already clipped), the SAME bits in every table kernel -- all of them inline
// it, whatever the storage format and the launch shape: left to the compiler, `b1 * m + (1 - b1) * g` is contracted into a
// fused multiply-add in one kernel and not in another (the 16-byte sweep and the row-list kernels were, the scalar sweeps
// were not), and from the second step on (moments no longer zero) the launch paths of one table stored moments, and with
// them weights, one ulp apart.  Contraction is off in here and the two fused operations are spelled out; every other
// operation is correctly rounded, hence unique.
__device__ __forceinline__ void adam_elem(float g, float& m, float& v, float& w, const AdamStep& s) {
#pragma clang fp contract(off)
  const float gm = (1.0f - s.b1) * g;
  const float gv = (1.0f - s.b2) * g * g;
  m = __builtin_fmaf(s.b1, m, gm);
  v = __builtin_fmaf(s.b2, v, gv);
  w = w - s.lr_t * m / (sqrtf(v) + s.eps);
}
// ... of the first VW elements of a 16-byte piece; g as loaded (not yet clipped)
template <int VW>
__device__ __forceinline__ void adam_piece(f32x4 g, f32x4& m, f32x4& v, f32x4& w, const AdamStep& s) {
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    float mk = m[k], vk = v[k], wk = w[k];
    adam_elem(g[k] * s.factor, mk, vk, wk, s);
    m[k] = mk;
    v[k] = vk;
    w[k] = wk;
  }
}

// ---- storage formats of a table [V, C]: element e / the four elements from e (a multiple of 4) read as fp32 and written
// back.  align4: what ld4 / st4 need of the table pointer(s) in bytes (the fp32 operands next to the table -- gradients,
// moments -- always need 16).
struct TableF32 {
  static constexpr int align4 = 16;
  float* t;
  __host__ __device__ TableF32(void* table, void* = nullptr) : t((float*)table) {}
  __device__ float ld(long e) const { return t[e]; }
  __device__ f32x4 ld4(long e) const { return ::ld4(t + e); }
  __device__ void st(long e, float w) const { t[e] = w; }
  __device__ void st4(long e, f32x4 w) const { ::st4(t + e, w); }
};
// bf16 (SURVEY 8d "bf16 tables"): widened, updated in fp32 with fp32 moments and gradients, and rounded to nearest-even when
// written back (6 + 2 x 2 bytes per element instead of 8 x 4: 28 against 32).  Without an fp32 master copy an update smaller
// than half a bf16 ulp of the weight (2^-9 relative) is lost; the parity test pins exactly this arithmetic.
struct TableBF16 {
  static constexpr int align4 = 8;
  __bf16* t;
  __host__ __device__ TableBF16(void* table, void* = nullptr) : t((__bf16*)table) {}
  __device__ float ld(long e) const { return (float)t[e]; }
  __device__ f32x4 ld4(long e) const { return __builtin_convertvector(*reinterpret_cast<const bf16x4_t*>(t + e), f32x4); }
  __device__ void st(long e, float w) const { t[e] = (__bf16)w; }
  __device__ void st4(long e, f32x4 w) const { *reinterpret_cast<bf16x4_t*>(t + e) = __builtin_convertvector(w, bf16x4_t); }
};
// bf16 with an exact fp32 master (common.h: hm_pack / hm_unpack): the table is the pair (hi = the bf16 values every other
// kernel reads, lo = 16-bit residual); the update rebuilds the fp32 master from both halves, updates it exactly as an fp32
// table and stores both halves back -- no update is lost to the bf16 rounding, and a step stays deterministic.  Per element
// g, m, v (4 + 4 bytes each) + hi (2 + 2) + lo (2 + 2) = 32 bytes: the fp32 update's traffic.
struct TableBF16M {
  static constexpr int align4 = 8;      // both halves
  unsigned short* hi;
  short* lo;
  __host__ __device__ TableBF16M(void* hi_, void* lo_) : hi((unsigned short*)hi_), lo((short*)lo_) {}
  __device__ float ld(long e) const { return hm_unpack(hi[e], lo[e]); }
  __device__ f32x4 ld4(long e) const {
    const u16x4_t h = *reinterpret_cast<const u16x4_t*>(hi + e);
    const i16x4_t l = *reinterpret_cast<const i16x4_t*>(lo + e);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = hm_unpack(h[k], l[k]);
    return r;
  }
  __device__ void st(long e, float w) const { hm_pack(w, hi[e], lo[e]); }
  __device__ void st4(long e, f32x4 w) const {
    u16x4_t h;
    i16x4_t l;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned short hk;
      short lk;
      hm_pack(w[k], hk, lk);
      h[k] = hk;
      l[k] = lk;
    }
    *reinterpret_cast<u16x4_t*>(hi + e) = h;
    *reinterpret_cast<i16x4_t*>(lo + e) = l;
  }
};

// ---- the loop skeletons
// Sweep of one table, dense or lazy (lazy != 0: only rows whose flag is set -- every row that got gradient through a lookup
// is also flagged as involved); clears the gradient of what it updates.  The flags are cleared by a second launch (every
// element of the sweep has read its flag by then).
template <class T>
__device__ __forceinline__ void adam_sweep(const T tab, float* __restrict__ grad, float* __restrict__ m,
                                           float* __restrict__ v, const unsigned char* __restrict__ flags, long V, int C,
                                           int lazy, const AdamStep& s) {
  const long total = V * C;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    if (lazy && !flags[e / C]) continue;
    float mm = m[e], vv = v[e], w = tab.ld(e);
    adam_elem(grad[e] * s.factor, mm, vv, w, s);
    m[e] = mm;
    v[e] = vv;
    tab.st(e, w);
    grad[e] = 0.f;
  }
}

// The same sweep for tables whose rows are multiples of four values (all of the reference's): one 16-byte access per
// thread and operand (8 bytes of a bf16 table or half), 32-bit index arithmetic (the scalar form divides a 64-bit element
// index by C per element), and the loads of two grid strides issued together from clamped addresses, selected by the row
// flags afterwards -- a load behind `if (flag)` leaves only once the flag has arrived, one dependent round trip per element
// of the stride loop.  Measured at configs[1] (5 M values in four tables, on the tail of the step): the Adam sweep 32 -> 27 us
// -- closer to its traffic (~70 MB through the L2 / Infinity Cache) than to its latency chain.  Fewer than 2^31 values;
// blocks of 256 threads; no LDS (csrc/multi.hip: tables_reg_multi_v4_kernel says why).
template <class T>
__device__ __forceinline__ void adam_sweep_v4(const T tab, float* __restrict__ grad, float* __restrict__ mp,
                                              float* __restrict__ vp, unsigned char* __restrict__ flags, long V, int C,
                                              int lazy, const AdamStep& s) {
  const unsigned QC = (unsigned)C >> 2, total = (unsigned)V * QC;
  const unsigned stride = gridDim.x * 256u;
  for (unsigned q0 = blockIdx.x * 256u + threadIdx.x; q0 < total; q0 += 2u * stride) {
    bool f[2];
    f32x4 g[2], m[2], v[2], w[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned q = q0 + (unsigned)u * stride, qs = q < total ? q : 0u;
      f[u] = q < total && (!lazy || flags[qs / QC]);
      g[u] = ld4(grad + 4L * qs); m[u] = ld4(mp + 4L * qs); v[u] = ld4(vp + 4L * qs);
      w[u] = tab.ld4(4L * qs);
      // dense Adam does not read the row flags: the thread of a row's first chunk clears the row's flag here and the
      // separate clearing launch is dropped (lazy Adam: every chunk of a row reads the flag first -- the second launch stays)
      if (!lazy && q < total && q % QC == 0) flags[q / QC] = 0;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!f[u]) continue;
      const long e = 4L * (q0 + (unsigned)u * stride);
      adam_piece<4>(g[u], m[u], v[u], w[u], s);
      st4(mp + e, m[u]);
      st4(vp + e, v[u]);
      tab.st4(e, w[u]);
      st4(grad + e, f32x4{0.f, 0.f, 0.f, 0.f});
    }
  }
}

// LazyAdam over the listed rows (ids / count from clsr_flags_compact: the involved rows of a huge table); clears their
// gradient rows and flags.  VW = floats per lane and access (4 when C % 4 == 0: 16-byte pieces of the 128-512 B rows, 4x
// fewer dependent id loads and address computations; random rows are HBM latency bound, so bytes in flight per lane matter).
// UN pieces per lane and trip: their 4 * UN loads are issued before the first one is used (random 384-byte rows of a
// 38 GB table: the update is bound by how many row reads are in flight; UN = 1 ran at 4.4-4.7 TB/s); a piece past the end
// (!ok) loads from the trip's first address.
template <class T, int VW, int UN>
__global__ void __launch_bounds__(256) table_adam_rows_kernel(
    const T tab, float* __restrict__ grad_table, float* __restrict__ m, float* __restrict__ v,
    unsigned char* __restrict__ flags, const int* __restrict__ ids, const int* __restrict__ count, int C,
    const double* __restrict__ sumsq, int sumsq_stride, int nsum, float clip_norm,
    const double* __restrict__ adam_state, float b1, float b2, float eps) {
  AdamStep s;
  if (!adam_begin(s, sumsq, sumsq_stride, nsum, clip_norm, adam_state, b1, b2, eps)) return;
  const int QC = C / VW;
  const long total = (long)count[0] * QC;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < total; i0 += stride * UN) {
    long e[UN], row[UN];
    int q[UN];
    bool ok[UN];
    f32x4 g[UN], mo[UN], vo[UN], po[UN];     // (VW = 1: element 0 only)
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
        g[u] = ld4(grad_table + e[u]); mo[u] = ld4(m + e[u]); vo[u] = ld4(v + e[u]); po[u] = tab.ld4(e[u]);
      } else {
        g[u][0] = grad_table[e[u]]; mo[u][0] = m[e[u]]; vo[u][0] = v[e[u]]; po[u][0] = tab.ld(e[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      adam_piece<VW>(g[u], mo[u], vo[u], po[u], s);
      if (!ok[u]) continue;
      if (VW == 4) {
        st4(m + e[u], mo[u]); st4(v + e[u], vo[u]); tab.st4(e[u], po[u]); st4(grad_table + e[u], f32x4{0.f, 0.f, 0.f, 0.f});
      } else {
        m[e[u]] = mo[u][0]; v[e[u]] = vo[u][0]; tab.st(e[u], po[u][0]); grad_table[e[u]] = 0.f;
      }
      if (q[u] == 0) flags[row[u]] = 0;
    }
  }
}
