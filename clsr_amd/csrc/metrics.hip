// Evaluation metrics on the device (gfx950): the scores of a whole validation / test file stay in HBM and only a
// handful of doubles come back.
//
// Reference: reco_utils/recommender/deeprec/deeprec_utils.py:554-821 (mrr_score, ndcg_score, hit_score, cal_metric,
// cal_weighted_metric) as called by SequentialBaseModel.run_eval / run_weighted_eval
// (models/sequential/sequential_base_model.py:204-292): auc + logloss over all lines, mean_mrr / ndcg@k / hit@k /
// group_auc over groups of 1 + num_ngs consecutive lines, rmse / acc / f1 and the mean fusion weight from one reduction
// over all lines, and the user-weighted wauc / wmrr / whit@k / wndcg@k: per-user values weighted by the user's line count.
//
// No sort of the scores anywhere (the lines are grouped by user id with the stable radix sort of csrc/segsum.hip, any
// non-negative int32 id): ROC-AUC with averaged tie ranks equals (#{pos > neg} + 0.5 #{pos == neg}) / (n_pos n_neg) --
// integer pair counts, exact -- and a positive's rank inside its group is a count as well.  Pair counting is P x N work for
// the global AUC (1e10 compare-and-count operations for a 1M-line test file: milliseconds on 256 CUs) and
// P_u x n_u inside a user / a group.  Rank ties (equal scores inside a group) break like a STABLE ascending sort read
// backwards: among equal scores the LATER line ranks first.  (numpy's default argsort, which the reference uses, is
// not stable above 16 elements, so the reference itself does not define that order.)
#include "common.h"
#include "clsr_hip.h"

typedef unsigned long long u64;

__device__ __forceinline__ double clip_d(double p, double lo, double hi) { return p < lo ? lo : (p > hi ? hi : p); }

// Order-independent accumulation of the per-block partial sums: double atomics add in whatever order the blocks
// finish, and a metric that sits exactly on a 4-decimal rounding boundary (0.58125: small test files produce such
// ratios) then rounds either way from run to run.  The partials are added as 64-bit FIXED-POINT integers instead
// (integer addition commutes exactly); a one-block kernel converts the slots back to doubles.  The slots must be
// zero on entry (the bit pattern of 0.0 is the integer 0) and hold the final sums on return.
__device__ __forceinline__ void fx_add(double* slot, double v, double scale) {
  atomicAdd(reinterpret_cast<u64*>(slot), (u64)__double2ll_rn(v * scale));
}
__global__ void fx_finalize_kernel(double* out, int n, double inv_scale) {
  const int i = threadIdx.x;
  if (i < n) out[i] = (double)(long long)reinterpret_cast<const u64*>(out)[i] * inv_scale;
}
static void fx_finalize(double* out, int n, double scale, hipStream_t s) {
  hipLaunchKernelGGL(fx_finalize_kernel, dim3(1), dim3(64), 0, s, out, n, 1.0 / scale);
}
// ---- partial forms (evaluation sharded over data-parallel ranks): `*_part(part, nparts)` does one share of the work
// over the same full arrays and leaves every accumulator -- fixed-point slots, pair counts, `err` counters (64-bit in
// this form) -- as a raw integer; the shares of all parts, added as integers, are the bits the whole entry leaves
// before its own conversion, and clsr_eval_finalize converts them once.  A kernel that rounds ONE sum per block (or per
// wave) to fixed point keeps its grid: part p runs the blocks [blocks p / nparts, blocks (p + 1) / nparts) of the
// whole launch (vb0 = the first of them, vgrid = blocks), so every block meets the elements it meets in the whole
// launch and rounds the same partial sum.  A part without a block launches nothing.
static inline void part_blocks(int blocks, int part, int nparts, int* vb0, int* nb) {
  *vb0 = (int)((long)blocks * part / nparts);
  *nb = (int)((long)blocks * (part + 1) / nparts) - *vb0;
}
#define CLSR_CHECK_PART() CLSR_CHECK_ARG(nparts > 0 && part >= 0 && part < nparts)
// err counters: int32 in the whole entries (their ABI), 64-bit slots of the packed accumulator in the partial ones
__device__ __forceinline__ void err_add(int* err, int i, int v, int wide) {
  if (wide) atomicAdd(reinterpret_cast<u64*>(err) + i, (u64)v);
  else atomicAdd(err + i, v);
}
#define FX_LOGLOSS 67108864.0              // 2^26: the sum is at most 27 N (N < 2^31 lines)
#define FX_GROUP 1073741824.0              // 2^30: sums of per-group values in [0, 1]
#define FX_WAUC 1152921504606846976.0      // 2^60: the weighted sum is at most 1
// 2^32: sums over the lines of terms in [0, 1] -- a squared error (predictions are sigmoid outputs and labels 0 / 1: the
// net refuses `method: regression`), alpha * label, label -- are at most N < 2^31, so the scaled sum stays below 2^63
#define FX_POINT 4294967296.0

// out[0] = sum over lines of -(y log p + (1 - y) log(1 - p)), p clipped to [1e-11, 1 - 1e-11] (cal_metric "logloss")
__global__ void __launch_bounds__(256) eval_logloss_kernel(const float* __restrict__ pred,
                                                           const float* __restrict__ labels, long N,
                                                           double* __restrict__ out, int vb0, int vgrid) {
  __shared__ double red[4];
  double s = 0.0;
  for (long e = (long)(vb0 + blockIdx.x) * 256 + threadIdx.x; e < N; e += (long)vgrid * 256) {
    const double p = clip_d((double)pred[e], 10e-12, 1.0 - 10e-12);
    const double y = (double)labels[e];
    s -= y * log(p) + (1.0 - y) * log(1.0 - p);
  }
  s = block256_sum_d(s, red);
  if (threadIdx.x == 0) fx_add(out, s, FX_LOGLOSS);
}

static void logloss_launch(const float* pred, const float* labels, long N, int part, int nparts, double* out,
                           hipStream_t s) {
  int blocks = clsr_cdiv(N, 256 * 8), vb0, nb;
  if (blocks > 2048) blocks = 2048;
  part_blocks(blocks, part, nparts, &vb0, &nb);
  if (nb > 0) hipLaunchKernelGGL(eval_logloss_kernel, dim3(nb), dim3(256), 0, s, pred, labels, N, out, vb0, blocks);
}

extern "C" int clsr_eval_logloss(const float* pred, const float* labels, long N, double* out, void* stream) {
  CLSR_CHECK_ARG(pred && labels && out && N > 0);
  logloss_launch(pred, labels, N, 0, 1, out, (hipStream_t)stream);
  fx_finalize(out, 1, FX_LOGLOSS, (hipStream_t)stream);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_eval_logloss_part(const float* pred, const float* labels, long N, int part, int nparts, void* acc,
                                      void* stream) {
  CLSR_CHECK_ARG(pred && labels && acc && N > 0);
  CLSR_CHECK_PART();
  logloss_launch(pred, labels, N, part, nparts, (double*)acc, (hipStream_t)stream);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// scores of the positive lines, compacted (any order); count[0] must be zero on entry
__global__ void __launch_bounds__(256) eval_compact_pos_kernel(const float* __restrict__ pred,
                                                               const float* __restrict__ labels, long N,
                                                               float* __restrict__ pos, int* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  for (long e0 = (long)blockIdx.x * 256; e0 < N; e0 += (long)gridDim.x * 256) {
    const long e = e0 + threadIdx.x;
    const bool on = e < N && labels[e] == 1.0f;
    const u64 m = __ballot(on);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(count, __popcll(m));
    base = __shfl(base, 0, 64);
    if (on) pos[base + __popcll(m & ((1ull << lane) - 1ull))] = pred[e];
  }
}

extern "C" int clsr_eval_compact_pos(const float* pred, const float* labels, long N, float* pos_out, int* count,
                                     void* stream) {
  CLSR_CHECK_ARG(pred && labels && pos_out && count && N > 0);
  CLSR_CHECK_SUPPORTED(N < (1L << 31));
  int blocks = clsr_cdiv(N, 256 * 4);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(eval_compact_pos_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred, labels, N, pos_out,
                     count);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// out[0] += #{(p, n): pos_p > neg_n}, out[1] += #{pos_p == neg_n}, out[2] += number of negative lines
#define AUC_NPT 4       // negatives per thread
#define AUC_PT 2048     // positives per LDS tile
__global__ void __launch_bounds__(256) eval_auc_pairs_kernel(const float* __restrict__ pred,
                                                             const float* __restrict__ labels, long N,
                                                             const float* __restrict__ pos,
                                                             const int* __restrict__ count, u64* __restrict__ out,
                                                             int vb0, int vgrid) {
  __shared__ float ps[AUC_PT];
  __shared__ u64 red[3][4];
  const int P = count[0];
  u64 gt = 0, eq = 0, nneg = 0;
  for (long e0 = (long)(vb0 + blockIdx.x) * (256 * AUC_NPT); e0 < N; e0 += (long)vgrid * (256 * AUC_NPT)) {
    float s[AUC_NPT];
    bool neg[AUC_NPT];
#pragma unroll
    for (int u = 0; u < AUC_NPT; ++u) {
      const long e = e0 + u * 256 + threadIdx.x;
      neg[u] = e < N && labels[e] != 1.0f;
      s[u] = neg[u] ? pred[e] : INFINITY;     // +inf: no finite positive is greater or equal
      nneg += neg[u] ? 1 : 0;
    }
    for (int p0 = 0; p0 < P; p0 += AUC_PT) {
      const int pc = min(AUC_PT, P - p0);
      __syncthreads();
      for (int i = threadIdx.x; i < pc; i += 256) ps[i] = pos[p0 + i];
      __syncthreads();
      unsigned g[AUC_NPT] = {0, 0, 0, 0}, q[AUC_NPT] = {0, 0, 0, 0};
      for (int i = 0; i < pc; ++i) {
        const float v = ps[i];
#pragma unroll
        for (int u = 0; u < AUC_NPT; ++u) { g[u] += v > s[u] ? 1u : 0u; q[u] += v == s[u] ? 1u : 0u; }
      }
#pragma unroll
      for (int u = 0; u < AUC_NPT; ++u) { gt += g[u]; eq += q[u]; }
    }
  }
  // block reduction of three 64-bit counters
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 v[3] = {gt, eq, nneg};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (lane == 0) red[k][wave] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const u64 t = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    if (t) atomicAdd(out + threadIdx.x, t);
  }
}

extern "C" int clsr_eval_auc_pairs(const float* pred, const float* labels, long N, const float* pos,
                                   const int* count, void* out_u64x3, void* stream) {
  return clsr_eval_auc_pairs_part(pred, labels, N, pos, count, 0, 1, out_u64x3, stream);
}

// pos / count: ALL positives of the file (every part compacts them itself); the part counts the pairs of its own lines
extern "C" int clsr_eval_auc_pairs_part(const float* pred, const float* labels, long N, const float* pos,
                                        const int* count, int part, int nparts, void* acc_u64x3, void* stream) {
  CLSR_CHECK_ARG(pred && labels && pos && count && acc_u64x3 && N > 0);
  CLSR_CHECK_PART();
  int blocks = clsr_cdiv(N, 256 * AUC_NPT), vb0, nb;
  if (blocks > 4096) blocks = 4096;
  part_blocks(blocks, part, nparts, &vb0, &nb);
  if (nb > 0)
    hipLaunchKernelGGL(eval_auc_pairs_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, pred, labels, N, pos, count,
                       (u64*)acc_u64x3, vb0, blocks);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---- group metrics: one wave per group of G consecutive lines
// out[0] += mrr, out[1] += group_auc, out[2 + i] += ndcg@ks[i], out[2 + nk + i] += hit@ks[i]; err[0] += groups without
// a positive or without a negative (the reference raises / divides by zero there)
#define GM_MAXK 8
struct GroupMetricArgs {
  const float* pred; const float* labels; long n_groups; int G; int nk; int ks[GM_MAXK]; int want_auc;
  double* out; int* err;
  int vb0, vgrid, err_wide;     // this launch = the blocks [vb0, vb0 + gridDim.x) of a launch of vgrid blocks (part_blocks)
};

__global__ void __launch_bounds__(256) eval_group_metrics_kernel(GroupMetricArgs a) {
  extern __shared__ float gs[];   // [4 waves][G] scores, then [4][G] labels
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = a.G;
  float* sc = gs + (long)wave * G;
  float* lb = gs + (long)4 * G + (long)wave * G;
  double acc[2 + 2 * GM_MAXK];
#pragma unroll
  for (int i = 0; i < 2 + 2 * GM_MAXK; ++i) acc[i] = 0.0;
  int bad = 0;
  for (long grp = (long)(a.vb0 + blockIdx.x) * 4 + wave; grp < a.n_groups; grp += (long)a.vgrid * 4) {
    const float* p = a.pred + grp * G;
    const float* l = a.labels + grp * G;
    for (int i = lane; i < G; i += 64) { sc[i] = p[i]; lb[i] = l[i]; }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    // every lane takes the lines i = lane, lane + 64, ...; positives compute their rank by a count over the group
    double mrr = 0.0, dcg[GM_MAXK], hit[GM_MAXK];
#pragma unroll
    for (int k = 0; k < GM_MAXK; ++k) { dcg[k] = 0.0; hit[k] = 0.0; }
    int npos = 0;
    u64 gt = 0, eq = 0;
    for (int i = lane; i < G; i += 64) {
      if (lb[i] != 1.0f) continue;
      ++npos;
      const float s = sc[i];
      int above = 0;
      for (int j = 0; j < G; ++j) {
        const float t = sc[j];
        above += (t > s || (t == s && j > i)) ? 1 : 0;
        if (a.want_auc && lb[j] != 1.0f) { gt += s > t ? 1 : 0; eq += s == t ? 1 : 0; }
      }
      const int rank = above + 1;
      mrr += 1.0 / (double)rank;
#pragma unroll
      for (int k = 0; k < GM_MAXK; ++k)
        if (k < a.nk && rank <= a.ks[k]) { dcg[k] += 1.0 / log2((double)rank + 1.0); hit[k] = 1.0; }
    }
    // wave reductions
    mrr = wave_sum_d(mrr);
    int np_all = npos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) np_all += __shfl_xor(np_all, o, 64);
    double gtd = (double)gt, eqd = (double)eq;
    gtd = wave_sum_d(gtd);
    eqd = wave_sum_d(eqd);
    const int nneg = G - np_all;
    if (np_all == 0 || (a.want_auc && nneg == 0)) ++bad;
    if (np_all > 0) {
      acc[0] += mrr / (double)np_all;
      if (a.want_auc && nneg > 0) acc[1] += (gtd + 0.5 * eqd) / ((double)np_all * (double)nneg);
#pragma unroll
      for (int k = 0; k < GM_MAXK; ++k) {
        if (k < a.nk) {
          const double d = wave_sum_d(dcg[k]);
          double h = hit[k];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) h = fmax(h, __shfl_xor(h, o, 64));
          double ideal = 0.0;
          const int kk = min(min(a.ks[k], G), np_all);
          for (int r = 1; r <= kk; ++r) ideal += 1.0 / log2((double)r + 1.0);
          acc[2 + k] += d / ideal;
          acc[2 + a.nk + k] += h;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    for (int i = 0; i < 2 + 2 * a.nk; ++i)
      if (acc[i] != 0.0) fx_add(a.out + i, acc[i], FX_GROUP);
    if (bad) err_add(a.err, 0, bad, a.err_wide);
  }
}

static int group_metrics_launch(const float* pred, const float* labels, long n_groups, int G, const int* ks_host, int nk,
                                int want_auc, int part, int nparts, double* out, int* err, int err_wide, hipStream_t s) {
  CLSR_CHECK_ARG(pred && labels && out && err && n_groups > 0 && G > 0 && nk >= 0 && (nk == 0 || ks_host));
  CLSR_CHECK_SUPPORTED(nk <= GM_MAXK && G <= 4096);
  CLSR_CHECK_PART();
  GroupMetricArgs a;
  a.pred = pred; a.labels = labels; a.n_groups = n_groups; a.G = G; a.nk = nk; a.want_auc = want_auc;
  a.out = out; a.err = err; a.err_wide = err_wide;
  for (int i = 0; i < GM_MAXK; ++i) a.ks[i] = i < nk ? ks_host[i] : 0;
  int blocks = clsr_cdiv(n_groups, 4), nb;
  if (blocks > 4096) blocks = 4096;
  a.vgrid = blocks;
  part_blocks(blocks, part, nparts, &a.vb0, &nb);
  if (nb > 0)
    hipLaunchKernelGGL(eval_group_metrics_kernel, dim3(nb), dim3(256), (size_t)8 * G * sizeof(float), s, a);
  return CLSR_OK;
}

extern "C" int clsr_eval_group_metrics(const float* pred, const float* labels, long n_groups, int G, const int* ks_host,
                                       int nk, int want_auc, double* out, int* err, void* stream) {
  const int rc = group_metrics_launch(pred, labels, n_groups, G, ks_host, nk, want_auc, 0, 1, out, err, 0,
                                      (hipStream_t)stream);
  if (rc != CLSR_OK) return rc;
  fx_finalize(out, 2 + 2 * nk, FX_GROUP, (hipStream_t)stream);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// whole groups only: a group is never split.  acc: 2 + 2 nk slots, err_i64: one 64-bit counter
extern "C" int clsr_eval_group_metrics_part(const float* pred, const float* labels, long n_groups, int G,
                                            const int* ks_host, int nk, int want_auc, int part, int nparts, void* acc,
                                            void* err_i64, void* stream) {
  const int rc = group_metrics_launch(pred, labels, n_groups, G, ks_host, nk, want_auc, part, nparts, (double*)acc,
                                      (int*)err_i64, 1, (hipStream_t)stream);
  if (rc != CLSR_OK) return rc;
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---- wauc over the buckets of the COUNTING sort (clsr_sort_ids_multi on the user ids: perm + the end offset of every
// bucket; one bucket = one user only for ids below 2^18 -- device_metrics.py uses clsr_eval_user_metrics below), one
// wave per user: out[0] += (n_u / N) * roc_auc(user u); err[0] += users whose lines are all one class
#define UA_PT 256
__global__ void __launch_bounds__(256) eval_user_auc_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ labels,
                                                            const int* __restrict__ perm, const int* __restrict__ ends,
                                                            int nb, long N, double* __restrict__ out,
                                                            int* __restrict__ err) {
  __shared__ float ps[4][UA_PT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  int bad = 0;
  for (long b = (long)blockIdx.x * 4 + wave; b < nb; b += (long)gridDim.x * 4) {
    const int lo = b ? ends[b - 1] : 0, hi = ends[b];
    const int n = hi - lo;
    if (n <= 0) continue;
    // positives of the segment, UA_PT at a time, against every negative of the segment
    u64 gt = 0, eq = 0;
    int npos = 0, done = 0;     // done: positives consumed so far (in segment order)
    while (true) {
      // gather the next UA_PT positives: a wave-wide ordered scan over the segment
      int got = 0, seen = 0;
      for (int i0 = 0; i0 < n && got < UA_PT; i0 += 64) {
        const int i = i0 + lane;
        const bool on = i < n && labels[perm[lo + i]] == 1.0f;
        const u64 m = __ballot(on);
        const int before = seen + __popcll(m & ((1ull << lane) - 1ull));   // index of this positive in the segment
        if (on && before >= done && before - done < UA_PT) ps[wave][before - done] = pred[perm[lo + i]];
        seen += __popcll(m);
        got = min(UA_PT, max(0, seen - done));
      }
      if (done == 0) {        // total number of positives: finish the scan once
        int tot = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
          const int i = i0 + lane;
          tot += __popcll(__ballot(i < n && labels[perm[lo + i]] == 1.0f));
        }
        npos = tot;
      }
      __builtin_amdgcn_wave_barrier();
      __threadfence_block();
      const int pc = min(UA_PT, npos - done);
      if (pc <= 0) break;
      for (int i = lane; i < n; i += 64) {
        const int row = perm[lo + i];
        if (labels[row] == 1.0f) continue;
        const float s = pred[row];
        unsigned g = 0, q = 0;
        for (int k = 0; k < pc; ++k) { const float v = ps[wave][k]; g += v > s ? 1u : 0u; q += v == s ? 1u : 0u; }
        gt += g; eq += q;
      }
      done += pc;
      __builtin_amdgcn_wave_barrier();
      if (done >= npos) break;
    }
    double gtd = wave_sum_d((double)gt), eqd = wave_sum_d((double)eq);
    const int nneg = n - npos;
    if (npos == 0 || nneg == 0) { ++bad; continue; }
    acc += ((double)n / (double)N) * (gtd + 0.5 * eqd) / ((double)npos * (double)nneg);
  }
  if (lane == 0) {
    if (acc != 0.0) fx_add(out, acc, FX_WAUC);
    if (bad) atomicAdd(err, bad);
  }
}

extern "C" int clsr_eval_user_auc(const float* pred, const float* labels, const int* perm, const int* ends, int nb,
                                  long N, double* out, int* err, void* stream) {
  CLSR_CHECK_ARG(pred && labels && perm && ends && out && err && nb > 0 && N > 0);
  int blocks = clsr_cdiv(nb, 4);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(eval_user_auc_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred, labels, perm, ends,
                     nb, N, out, err);
  fx_finalize(out, 1, FX_WAUC, (hipStream_t)stream);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---- user segments: keys = the user ids of the lines in ascending order (clsr_sort_ids_stable_multi: equal ids stay in
// line order).  starts[0 .. count[0]) = the entries e with e == 0 or keys[e] != keys[e - 1], in ANY order; count[0] must be
// zero on entry and never travels to the host: the consumer strides over it.
__global__ void __launch_bounds__(256) eval_user_segments_kernel(const int* __restrict__ keys, long N,
                                                                 int* __restrict__ starts, int* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  for (long e0 = (long)blockIdx.x * 256; e0 < N; e0 += (long)gridDim.x * 256) {
    const long e = e0 + threadIdx.x;
    const bool on = e < N && (e == 0 || keys[e] != keys[e - 1]);
    const u64 m = __ballot(on);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(count, __popcll(m));
    base = __shfl(base, 0, 64);
    if (on) starts[base + __popcll(m & ((1ull << lane) - 1ull))] = (int)e;
  }
}

extern "C" int clsr_eval_user_segments(const int* keys, long N, int* starts, int* count, void* stream) {
  CLSR_CHECK_ARG(keys && starts && count && N > 0);
  CLSR_CHECK_SUPPORTED(N < (1L << 31) - 2048);
  int blocks = clsr_cdiv(N, 256 * 4);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(eval_user_segments_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, keys, N, starts, count);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---- user-weighted metrics: one wave per user segment.  With w = n_u / N, P_u positives and the rank of a positive line
// i = 1 + #{j in u: s_j > s_i or (s_j == s_i and line_j > line_i)} (line = the index in the file = perm, so the rule does
// not depend on the order inside the segment; the group kernel's rule):
//   out[0] += w roc_auc(u)   out[1] += w (sum 1 / rank) / P_u   out[2 + i] += w dcg@ks[i] / ideal dcg@ks[i]
//   out[2 + GM_MAXK + i] += w [any rank <= ks[i]];   err[0] += users whose lines are all one class (want_auc only),
//   err[1] += users without a positive line (they add nothing to out[1 ..]; the host path yields NaN for mrr / ndcg there).
// The wave takes the user's positives 64 at a time, one per lane (a cursor walks the segment once), and streams ALL lines
// of the user past them through an LDS tile of 64 lines: a positive's rank count (RANK: ONE 64-bit compare per line, key =
// order-preserving score bits above the line index) and its (positive > negative, positive == negative) pair counts (AUC:
// a positive line of the tile holds +inf) come out of the same loop; a wauc-only request pays for the pair counts alone.
// The tile after next is already on its way while a tile is compared (a user with very many lines is ONE wave: nothing
// else hides the two dependent trips perm -> pred / labels).  P_u x n_u / 64 steps per user, any n_u and P_u.  Every
// user's values are rounded to fixed point on their own and added as integers: which wave meets which user (the start
// list is unordered) does not show.
struct UserMetricArgs {
  const float* pred; const float* labels; const int* perm; const int* keys; const int* starts; const int* count;
  long N; int nk; int ks[GM_MAXK];
  double* out; int* err;
  int part, nparts;     // PART: the users with id % nparts == part -- the same users on every rank, whatever the order of starts
};
__device__ __forceinline__ u64 fx_wauc(double v) { return (u64)__double2ll_rn(v * FX_WAUC); }
// s > t or (s == t and line_s > line_t)  <=>  um_key(s, line_s) > um_key(t, line_t)   (finite scores, -0 == +0)
__device__ __forceinline__ u64 um_key(float s, int line) {
  const unsigned b = __float_as_uint(s + 0.0f);
  return ((u64)(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u)) << 32) | (unsigned)line;
}
// LDS written by one lane of the wave and read by another: LDS operations of a wave execute in order, so only the
// compiler has to be held (no wait for the global loads in flight, which a workgroup fence would add)
__device__ __forceinline__ void um_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// PART: the partial form (share of the users, 64-bit err counters); the whole entry keeps instances without it, so its
// code -- one wave walks the heavy user's lines alone: every instruction of that loop shows -- is what it was
template <bool AUC, bool RANK, bool PART>
__global__ void __launch_bounds__(256) eval_user_metrics_kernel(UserMetricArgs a) {
  __shared__ float tn[4][64];   // tile: score of a NEGATIVE line, +inf for a positive one (hand-over: a positive's score)
  __shared__ u64 tk[4][64];     // tile: rank key of a line (hand-over: a positive's line)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* sn = tn[wave];
  u64* sk = tk[wave];
  const int nseg = a.count[0];
  const u64 below = (1ull << lane) - 1ull;
  u64 acc[2 + 2 * GM_MAXK];
#pragma unroll
  for (int i = 0; i < 2 + 2 * GM_MAXK; ++i) acc[i] = 0;
  int bad = 0, nopos = 0;
  for (long b = (long)blockIdx.x * 4 + wave; b < nseg; b += (long)gridDim.x * 4) {
    const int lo = __builtin_amdgcn_readfirstlane(a.starts[b]);      // (the same in every lane: scalar loop bounds)
    const int key = a.keys[lo];
    if (PART && (unsigned)key % (unsigned)a.nparts != (unsigned)a.part) continue;
    int hi = (int)a.N;        // the segment ends at the first later entry with another key
    for (long i0 = (long)lo + 1; i0 < a.N; i0 += 64) {
      const long i = i0 + lane;
      const u64 m = __ballot(i < a.N && a.keys[i] != key);
      if (m) { hi = (int)(i0 + (__ffsll((long long)m) - 1)); break; }
    }
    const int n = __builtin_amdgcn_readfirstlane(hi - lo);
    u64 gt = 0, eq = 0;
    double mrr = 0.0, dcg[GM_MAXK];
#pragma unroll
    for (int k = 0; k < GM_MAXK; ++k) dcg[k] = 0.0;
    int hits = 0, npos = 0;     // hits: bit k = a positive of this lane ranks within ks[k]
    int cur = 0, skip = 0;      // cursor of the positive scan: chunk start in the segment, positives of it already taken
    while (true) {
      // the next (up to) 64 positives of the segment, in segment order: number t of them -> lane t
      um_wave_sync();
      int got = 0;
      while (cur < n && got < 64) {
        const int i = cur + lane;
        int row = 0;
        bool on = false;
        if (i < n) { row = a.perm[lo + i]; on = a.labels[row] == 1.0f; }
        const u64 m = __ballot(on);
        const int before = __popcll(m & below), idx = got + before - skip;
        if (on && before >= skip && idx < 64) { sn[idx] = a.pred[row]; sk[idx] = (u64)(unsigned)row; }
        const int avail = __popcll(m) - skip;
        if (got + avail > 64) { skip += 64 - got; got = 64; }      // the rest of this chunk: next round
        else { got += avail; skip = 0; cur += 64; }
      }
      if (got == 0) break;
      npos += got;
      um_wave_sync();
      const bool have = lane < got;
      const float v = have ? sn[lane] + 0.0f : 0.0f;
      const u64 kv = um_key(v, have ? (int)sk[lane] : 0);
      int above = 0;
      unsigned g = 0, q = 0;
      // lines of the segment, 64 (one per lane) at a time: rowB = the rows of the tile after next,
      // (rowA, pA, yA) = the next tile
      int rowA = lane < n ? a.perm[lo + lane] : -1;
      int rowB = 64 + lane < n ? a.perm[lo + 64 + lane] : -1;
      float pA = 0.0f, yA = 0.0f;
      if (rowA >= 0) { pA = a.pred[rowA]; yA = a.labels[rowA]; }
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int cnt = min(64, n - j0);
        um_wave_sync();
        if (lane < cnt) {
          if (AUC) sn[lane] = yA == 1.0f ? INFINITY : pA + 0.0f;
          if (RANK) sk[lane] = um_key(pA, rowA);
        }
        rowA = rowB;
        rowB = j0 + 128 + lane < n ? a.perm[lo + j0 + 128 + lane] : -1;
        if (rowA >= 0) { pA = a.pred[rowA]; yA = a.labels[rowA]; }
        um_wave_sync();
        if (have) {
          if (cnt == 64) {      // a whole tile: wide LDS reads, compares of several lines in flight
#pragma unroll 16
            for (int j = 0; j < 64; ++j) {
              if (RANK) above += sk[j] > kv ? 1 : 0;
              if (AUC) { const float t = sn[j]; g += v > t ? 1u : 0u; q += v == t ? 1u : 0u; }
            }
          } else {
            for (int j = 0; j < cnt; ++j) {
              if (RANK) above += sk[j] > kv ? 1 : 0;
              if (AUC) { const float t = sn[j]; g += v > t ? 1u : 0u; q += v == t ? 1u : 0u; }
            }
          }
        }
      }
      if (have) {
        gt += g; eq += q;
        if (RANK) {
          const int rank = above + 1;
          mrr += 1.0 / (double)rank;
#pragma unroll
          for (int k = 0; k < GM_MAXK; ++k)
            if (k < a.nk && rank <= a.ks[k]) { dcg[k] += 1.0 / log2((double)rank + 1.0); hits |= 1 << k; }
        }
      }
      if (got < 64) break;      // (the scan reached the end of the segment)
    }
    const double w = (double)n / (double)a.N;
    const int nneg = n - npos;
    if (AUC) {
      const double gtd = wave_sum_d((double)gt), eqd = wave_sum_d((double)eq);
      if (npos == 0 || nneg == 0) ++bad;
      else acc[0] += fx_wauc(w * ((gtd + 0.5 * eqd) / ((double)npos * (double)nneg)));
    }
    if (npos == 0) { ++nopos; continue; }
    if (RANK) {
      acc[1] += fx_wauc(w * (wave_sum_d(mrr) / (double)npos));
#pragma unroll
      for (int k = 0; k < GM_MAXK; ++k) {
        if (k < a.nk) {
          const double d = wave_sum_d(dcg[k]);
          double ideal = 0.0;
          const int kk = min(min(a.ks[k], n), npos);
          for (int r = 1 + lane; r <= kk; r += 64) ideal += 1.0 / log2((double)r + 1.0);
          ideal = wave_sum_d(ideal);
          acc[2 + k] += fx_wauc(w * (d / ideal));
          if (__ballot((hits >> k) & 1)) acc[2 + GM_MAXK + k] += fx_wauc(w);
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 2 + 2 * GM_MAXK; ++i)
      if (acc[i]) atomicAdd(reinterpret_cast<u64*>(a.out) + i, acc[i]);
    if (bad) err_add(a.err, 0, bad, PART);
    if (nopos) err_add(a.err, 1, nopos, PART);
  }
}

static int user_metrics_launch(const float* pred, const float* labels, const int* perm, const int* keys,
                               const int* starts, const int* count, long N, const int* ks_host, int nk, int want_auc,
                               int want_rank, int part, int nparts, double* out, int* err, bool partial, hipStream_t s) {
  CLSR_CHECK_ARG(pred && labels && perm && keys && starts && count && out && err && N > 0 && nk >= 0 &&
                 (nk == 0 || ks_host) && (want_auc || want_rank) && (want_rank || nk == 0));
  CLSR_CHECK_SUPPORTED(nk <= GM_MAXK && N < (1L << 31) - 2048);
  CLSR_CHECK_PART();
  UserMetricArgs a;
  a.pred = pred; a.labels = labels; a.perm = perm; a.keys = keys; a.starts = starts; a.count = count;
  a.N = N; a.nk = nk; a.out = out; a.err = err; a.part = part; a.nparts = nparts;
  for (int i = 0; i < GM_MAXK; ++i) {
    CLSR_CHECK_ARG(i >= nk || ks_host[i] > 0);
    a.ks[i] = i < nk ? ks_host[i] : 0;
  }
  int blocks = clsr_cdiv(N, 4);      // at most one wave per line: the number of users stays on the device
  if (blocks > 4096) blocks = 4096;
#define UM_LAUNCH(AUC, RANK)                                                                                      \
  do {                                                                                                            \
    if (partial) hipLaunchKernelGGL((eval_user_metrics_kernel<AUC, RANK, true>), dim3(blocks), dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((eval_user_metrics_kernel<AUC, RANK, false>), dim3(blocks), dim3(256), 0, s, a);       \
  } while (0)
  if (want_auc && want_rank) UM_LAUNCH(true, true);
  else if (want_auc) UM_LAUNCH(true, false);
  else UM_LAUNCH(false, true);
#undef UM_LAUNCH
  return CLSR_OK;
}

extern "C" int clsr_eval_user_metrics(const float* pred, const float* labels, const int* perm, const int* keys,
                                      const int* starts, const int* count, long N, const int* ks_host, int nk,
                                      int want_auc, int want_rank, double* out, int* err, void* stream) {
  const int rc = user_metrics_launch(pred, labels, perm, keys, starts, count, N, ks_host, nk, want_auc, want_rank, 0, 1,
                                     out, err, false, (hipStream_t)stream);
  if (rc != CLSR_OK) return rc;
  fx_finalize(out, 2 + 2 * GM_MAXK, FX_WAUC, (hipStream_t)stream);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// the users whose id is `part` modulo nparts (keys / perm / starts cover ALL lines: the stable sort makes keys and perm
// the same on every rank, the ORDER of starts is not -- so the share is a property of the user, not of a list position).
// acc: 18 slots, err_i64x2: two 64-bit counters
extern "C" int clsr_eval_user_metrics_part(const float* pred, const float* labels, const int* perm, const int* keys,
                                           const int* starts, const int* count, long N, const int* ks_host, int nk,
                                           int want_auc, int want_rank, int part, int nparts, void* acc,
                                           void* err_i64x2, void* stream) {
  const int rc = user_metrics_launch(pred, labels, perm, keys, starts, count, N, ks_host, nk, want_auc, want_rank, part,
                                     nparts, (double*)acc, (int*)err_i64x2, true, (hipStream_t)stream);
  if (rc != CLSR_OK) return rc;
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---- point statistics in one pass over the lines (cal_metric "rmse" / "acc" / "f1", cal_mean_alpha_metric):
// outd[0] += sum (label - pred)^2, outd[1] += sum alpha * label, outd[2] += sum label (the last two only with alpha);
// outu[0] += #{(pred >= 0.5) == label}, outu[1 .. 3] += TP, FP, FN at the threshold 0.5 (positive: label == 1)
__global__ void __launch_bounds__(256) eval_point_stats_kernel(const float* __restrict__ pred,
                                                               const float* __restrict__ labels,
                                                               const float* __restrict__ alpha, long N,
                                                               double* __restrict__ outd, u64* __restrict__ outu,
                                                               int vb0, int vgrid) {
  __shared__ double red[3][4];
  __shared__ u64 redu[4][4];
  double s[3] = {0.0, 0.0, 0.0};
  u64 c[4] = {0, 0, 0, 0};
  for (long e = (long)(vb0 + blockIdx.x) * 256 + threadIdx.x; e < N; e += (long)vgrid * 256) {
    const float p = pred[e], y = labels[e];
    const double d = (double)y - (double)p;
    s[0] += d * d;
    const bool pp = p >= 0.5f, lab = y == 1.0f;
    c[0] += (pp ? 1.0f : 0.0f) == y ? 1 : 0;
    c[1] += pp && lab ? 1 : 0;
    c[2] += pp && !lab ? 1 : 0;
    c[3] += !pp && lab ? 1 : 0;
    if (alpha) { s[1] += (double)alpha[e] * (double)y; s[2] += (double)y; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = block256_sum_d(s[k], red[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
    if (lane == 0) redu[k][wave] = c[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (s[k] != 0.0) fx_add(outd + k, s[k], FX_POINT);
  }
  if (threadIdx.x < 4) {
    const u64 t = redu[threadIdx.x][0] + redu[threadIdx.x][1] + redu[threadIdx.x][2] + redu[threadIdx.x][3];
    if (t) atomicAdd(outu + threadIdx.x, t);
  }
}

static int point_stats_launch(const float* pred, const float* labels, const float* alpha, long N, int part, int nparts,
                              double* out_d3, u64* out_u64x4, hipStream_t s) {
  CLSR_CHECK_ARG(pred && labels && out_d3 && out_u64x4 && N > 0);
  CLSR_CHECK_SUPPORTED(N < (1L << 31));
  CLSR_CHECK_PART();
  int blocks = clsr_cdiv(N, 256 * 8), vb0, nb;
  if (blocks > 2048) blocks = 2048;
  part_blocks(blocks, part, nparts, &vb0, &nb);
  if (nb > 0)
    hipLaunchKernelGGL(eval_point_stats_kernel, dim3(nb), dim3(256), 0, s, pred, labels, alpha, N, out_d3, out_u64x4,
                       vb0, blocks);
  return CLSR_OK;
}

extern "C" int clsr_eval_point_stats(const float* pred, const float* labels, const float* alpha, long N, double* out_d3,
                                     void* out_u64x4, void* stream) {
  const int rc = point_stats_launch(pred, labels, alpha, N, 0, 1, out_d3, (u64*)out_u64x4, (hipStream_t)stream);
  if (rc != CLSR_OK) return rc;
  fx_finalize(out_d3, 3, FX_POINT, (hipStream_t)stream);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_eval_point_stats_part(const float* pred, const float* labels, const float* alpha, long N, int part,
                                          int nparts, void* acc_d3, void* acc_u64x4, void* stream) {
  const int rc = point_stats_launch(pred, labels, alpha, N, part, nparts, (double*)acc_d3, (u64*)acc_u64x4,
                                    (hipStream_t)stream);
  if (rc != CLSR_OK) return rc;
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// the conversion every whole entry ends with, on its own: n <= 64 raw fixed-point slots of scale `scale`
// (CLSR_EVAL_FX_*) become doubles in place, after the shares of all parts have been added as integers
extern "C" int clsr_eval_finalize(void* acc, int n, int scale, void* stream) {
  CLSR_CHECK_ARG(acc && n > 0 && n <= 64 && scale >= 0 && scale <= 3);
  const double scales[4] = {FX_LOGLOSS, FX_GROUP, FX_WAUC, FX_POINT};
  fx_finalize((double*)acc, n, scales[scale], (hipStream_t)stream);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}
