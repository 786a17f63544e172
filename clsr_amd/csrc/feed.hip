// Training feeds built on the device from a resident column store (clsr_amd/resident.py).
//
// A training batch is a deterministic row gather: which file lines were drawn (sel) and which in-batch line every output
// row takes its item / category from (src) is all a batch carries; the padded histories, time features, lengths and ids of
// the file stay in HBM.  clsr_feed_build writes the tensors CLSRNet.upload would have filled (include/clsr_hip.h).
//
// Two launches.  feed_check_kernel (ONE workgroup) holds every sel against N and every src of the shard against n_sel,
// counts the histories longer than the contrastive threshold as an integer and writes denom; a bad index raises the sticky
// error words and the per-launch status instead.  feed_build_kernel reads that status first and writes nothing when it is
// set, so no index that failed the check is ever used as an address.  No atomics on floats, no LDS beyond two words.
#include "clsr_hip.h"
#include "common.h"

#include <limits.h>

#include <initializer_list>

typedef unsigned feed_u32x4 __attribute__((ext_vector_type(4)));

// the resident columns of a file (labels: evaluation stores only) and the tensors of a feed, as the kernels take them
struct FeedCols {
  const int* item_history; const int* item_cate_history; const float* time_from_first_action; const float* time_to_now;
  const int* lens; const int* users; const int* items; const int* cates; const float* labels;
};
struct FeedOuts {
  int* out_users; int* out_items; int* out_cates; int* out_item_history; int* out_item_cate_history;
  float* out_time_from_first_action; float* out_time_to_now; float* out_labels; int* out_users_rows; int* out_seq_len;
  float* out_denom;
};

// the arguments of one call as the kernels take them (by value)
struct FeedArgs : FeedCols, FeedOuts {
  const int* sel; const int* src;
  int* err;
  long N, n_sel, h0, n;
  int T, G, expanded, thr;
};

// The first ncols entries of a host column array (include/clsr_hip.h has the order) -> c; false if one is null.
static bool feed_cols(FeedCols& c, const void* const* p, int ncols) {
  const void* v[9] = {};
  bool ok = p != nullptr;
  for (int i = 0; ok && i < ncols; ++i) ok = (v[i] = p[i]) != nullptr;
  c = {(const int*)v[0], (const int*)v[1], (const float*)v[2], (const float*)v[3], (const int*)v[4],
       (const int*)v[5], (const int*)v[6], (const int*)v[7], (const float*)v[8]};
  return ok;
}

// A host output array -> o: the ten tensors of a training feed, or (rows) the eleven of an evaluation feed, whose
// users_rows may be null (a g == 1 feed has no such tensor); false if another one is null.
static bool feed_outs(FeedOuts& o, void* const* p, bool rows) {
  if (!p) return false;
  o = {(int*)p[0], (int*)p[1], (int*)p[2], (int*)p[3], (int*)p[4], (float*)p[5], (float*)p[6], (float*)p[7],
       rows ? (int*)p[8] : nullptr, (int*)p[rows ? 9 : 8], (float*)p[rows ? 10 : 9]};
  return o.out_users && o.out_items && o.out_cates && o.out_item_history && o.out_item_cate_history &&
         o.out_time_from_first_action && o.out_time_to_now && o.out_labels && o.out_seq_len && o.out_denom;
}

// 16-byte accesses where every row of T words starts on a 16-byte boundary on every side that is read or written in words
// of W (T = 50 does not)
static bool feed_wide(int T, std::initializer_list<const void*> sides) {
  uintptr_t a = 0;
  for (const void* p : sides) a |= (uintptr_t)p;
  return T % 4 == 0 && a % 16 == 0;
}
static bool feed_wide_rows(int T, const FeedCols& c, const FeedOuts& o) {
  return feed_wide(T, {c.item_history, c.item_cate_history, c.time_from_first_action, c.time_to_now, o.out_item_history,
                       o.out_item_cate_history, o.out_time_from_first_action, o.out_time_to_now});
}

// workgroups of 256 threads for `work` items, a thread each up to `cap` workgroups (grid-stride loops beyond)
static int feed_blocks(long work, long cap) {
  const long b = (work + 255) / 256;
  return (int)(b > cap ? cap : b);
}
enum { FEED_BIG_BLOCKS = 16384, FEED_SMALL_BLOCKS = 1024 };

// the 16-byte or the 4-byte instance of a kernel template on `blocks` workgroups of 256 threads
#define FEED_LAUNCH(kernel, wide, blocks, st, ...)                                                    \
  do {                                                                                                \
    if (wide)                                                                                         \
      hipLaunchKernelGGL(kernel<feed_u32x4>, dim3(blocks), dim3(256), 0, st, __VA_ARGS__);            \
    else                                                                                              \
      hipLaunchKernelGGL(kernel<unsigned>, dim3(blocks), dim3(256), 0, st, __VA_ARGS__);              \
    CLSR_CHECK_LAUNCH();                                                                              \
  } while (0)

enum { FEED_ERR_CODE = 0, FEED_ERR_INDEX = 1, FEED_ERR_VALUE = 2, FEED_ERR_LAUNCH = 3 };

// The two ends of a checker (ONE workgroup of 1024 threads).  feed_refuse, one thread: raise (code, index, *value) unless
// an earlier failure is still there, and set the launch status the builder reads first.  feed_accept, every thread, s_cnt
// zeroed before a barrier: count the shard's histories longer than thr as an integer, clear the status, write denom.
__device__ __forceinline__ void feed_refuse(int* err, int code, int index, const int* value) {
  if (err[FEED_ERR_CODE] == 0) {      // sticky: the first failure stays until clsr_feed_clear_error
    err[FEED_ERR_CODE] = code;
    err[FEED_ERR_INDEX] = index;
    err[FEED_ERR_VALUE] = *value;
  }
  err[FEED_ERR_LAUNCH] = 1;
}

__device__ __forceinline__ void feed_accept(const FeedArgs& d, int* s_cnt) {
  int cnt = 0;
  for (int i = threadIdx.x; i < (int)d.n; i += 1024) cnt += d.lens[d.sel[d.h0 + i]] > d.thr ? 1 : 0;
  if (cnt) atomicAdd(s_cnt, cnt);           // integer sum: the value does not depend on the order
  __syncthreads();
  if (threadIdx.x == 0) {
    d.err[FEED_ERR_LAUNCH] = 0;
    d.out_denom[0] = (float)((long)*s_cnt * d.G);
  }
}

__global__ void __launch_bounds__(1024) feed_check_kernel(FeedArgs d) {
  __shared__ int s_bad, s_cnt;
  if (threadIdx.x == 0) {
    s_bad = INT_MAX;
    s_cnt = 0;
  }
  __syncthreads();
  const int n_sel = (int)d.n_sel, nrow = (int)(d.n * d.G);
  const long row0 = d.h0 * d.G;
  // position of the first index that cannot be served: sel entries first, then the shard's src entries
  for (int i = threadIdx.x; i < n_sel; i += 1024)
    if ((unsigned)d.sel[i] >= (unsigned long)d.N) atomicMin(&s_bad, i);
  for (int j = threadIdx.x; j < nrow; j += 1024)
    if ((unsigned)d.src[row0 + j] >= (unsigned)n_sel) atomicMin(&s_bad, n_sel + j);
  __syncthreads();
  const int bad = s_bad;
  if (bad != INT_MAX) {
    if (threadIdx.x == 0)
      feed_refuse(d.err, bad < n_sel ? 1 : 2, bad < n_sel ? bad : bad - n_sel,
                  bad < n_sel ? d.sel + bad : d.src + row0 + (bad - n_sel));
    return;
  }
  feed_accept(d, &s_cnt);
}

// The file line an output row of the four history-level arrays is copied from: a training feed (lines sel[h0 ..), every
// line G times when expanded) and an evaluation chunk (every g-th line of keep[k0 ..)).
struct FeedTrainLine {
  const FeedArgs& d;
  __device__ __forceinline__ long operator()(long r) const { return d.sel[d.h0 + (d.expanded ? r / d.G : r)]; }
};
struct FeedEvalLine {
  const int* __restrict__ keep;
  int g;
  __device__ __forceinline__ long operator()(long h) const { return keep[h * g]; }
};

// W: one 4-byte word or four per access.  A row of T words is contiguous on both sides and consecutive lanes walk
// consecutive words of it; the four history-level arrays move together (four independent loads in flight per lane).
template <typename W, typename Line>
__device__ __forceinline__ void feed_move_rows(const FeedCols& cols, const FeedOuts& outs, const Line line_of, long nq,
                                               int Tq, int big_blocks) {
  const W* __restrict__ c0 = (const W*)cols.item_history;
  const W* __restrict__ c1 = (const W*)cols.item_cate_history;
  const W* __restrict__ c2 = (const W*)cols.time_from_first_action;
  const W* __restrict__ c3 = (const W*)cols.time_to_now;
  W* __restrict__ o0 = (W*)outs.out_item_history;
  W* __restrict__ o1 = (W*)outs.out_item_cate_history;
  W* __restrict__ o2 = (W*)outs.out_time_from_first_action;
  W* __restrict__ o3 = (W*)outs.out_time_to_now;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)big_blocks * 256) {
    const long r = q / Tq;
    const int c = (int)(q - r * Tq);
    const long s = line_of(r) * Tq + c;
    const W v0 = c0[s], v1 = c1[s], v2 = c2[s], v3 = c3[s];
    o0[q] = v0;
    o1[q] = v1;
    o2[q] = v2;
    o3[q] = v3;
  }
}

template <typename W>
__global__ void __launch_bounds__(256) feed_build_kernel(FeedArgs d, long nq, int Tq, int big_blocks) {
  if (d.err[FEED_ERR_LAUNCH]) return;
  const int G = d.G;
  if ((int)blockIdx.x < big_blocks) {
    feed_move_rows<W>(d, d, FeedTrainLine{d}, nq, Tq, big_blocks);
    return;
  }
  const long nrow = d.n * G, row0 = d.h0 * G;
  const long stride = (long)(gridDim.x - big_blocks) * 256;
  for (long b = (long)(blockIdx.x - big_blocks) * 256 + threadIdx.x; b < nrow; b += stride) {
    const long h = b / G;
    const int g = (int)(b - h * G);
    const int from = d.sel[d.src[row0 + b]];
    d.out_items[b] = d.items[from];
    d.out_cates[b] = d.cates[from];
    d.out_labels[b] = g == 0 ? 1.0f : 0.0f;
    const int own = d.sel[d.h0 + h];
    if (d.expanded) {
      d.out_users[b] = d.users[own];
      d.out_seq_len[b] = d.lens[own];
    } else if (g == 0) {
      d.out_users[h] = d.users[own];
      d.out_seq_len[h] = d.lens[own];
    }
  }
}

extern "C" int clsr_feed_build_max_group(void) { return 1024; }
extern "C" int clsr_feed_build_max_steps(void) { return 4096; }

extern "C" int clsr_feed_build_supported(long N, long n_sel, int T, int G) {
  return N >= 1 && N <= INT_MAX && n_sel >= 1 && T >= 1 && T <= clsr_feed_build_max_steps() && G >= 1 &&
         G <= clsr_feed_build_max_group() && n_sel * ((long)G + 1) < INT_MAX;
}

// The arguments of clsr_feed_build / clsr_feed_build_pos -> d, checked; `supported`: the entry point's own shape rule.
static int feed_train_args(FeedArgs& d, const void* const* cols_host, long N, const int* sel, long n_sel, const int* src,
                           long h0, long n, int T, int G, int expanded, int thr, void* const* outs_host, int* err,
                           int supported) {
  CLSR_CHECK_ARG(feed_cols(d, cols_host, 8));
  CLSR_CHECK_ARG(feed_outs(d, outs_host, false));
  CLSR_CHECK_ARG(sel && src && err);
  d.sel = sel, d.src = src, d.err = err;
  d.N = N, d.n_sel = n_sel, d.h0 = h0, d.n = n;
  d.T = T, d.G = G, d.expanded = expanded, d.thr = thr;
  CLSR_CHECK_SUPPORTED(supported);
  CLSR_CHECK_ARG(d.h0 >= 0 && d.n >= 1 && d.h0 + d.n <= d.n_sel);
  CLSR_CHECK_ARG(d.expanded == 0 || d.expanded == 1);
  return CLSR_OK;
}

extern "C" int clsr_feed_build(const void* const* cols_host, long N, const int* sel, long n_sel, const int* src, long h0,
                               long n, int T, int G, int expanded, int thr, void* const* outs_host, int* err, void* stream) {
  FeedArgs d;
  const int rc = feed_train_args(d, cols_host, N, sel, n_sel, src, h0, n, T, G, expanded, thr, outs_host, err,
                                 clsr_feed_build_supported(N, n_sel, T, G));
  if (rc != CLSR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(feed_check_kernel, dim3(1), dim3(1024), 0, st, d);
  CLSR_CHECK_LAUNCH();
  const bool wide = feed_wide_rows(d.T, d, d);
  const int Tq = wide ? d.T / 4 : d.T;
  const long nq = d.n * (d.expanded ? d.G : 1) * Tq;
  const int big = feed_blocks(nq, FEED_BIG_BLOCKS), small = feed_blocks(d.n * d.G, FEED_SMALL_BLOCKS);
  FEED_LAUNCH(feed_build_kernel, wide, big + small, st, d, nq, Tq, big);
  return CLSR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// NextItNet training feeds (NextItNetColumnIterator): a target per position.  The recipe is sel and psrc [n_sel, G - 1, T],
// the batch line every (line, negative, step) takes its item / category from; the columns are the LEFT-padded ones.
// The same protocol as above in three launches.  The shard's psrc is n (G - 1) T words (3.3 MB at 4096 x 4 x 50), too many
// for one workgroup: feed_scan_pos_kernel holds sel and the shard's psrc in slices and leaves the first position that cannot
// be served per workgroup (plain stores, no atomics on global memory); feed_check_pos_kernel (ONE workgroup) takes their
// minimum and raises the error words or -- everything passed -- writes denom and the batch's own targets bt[0 .. n_sel) =
// items[sel], bt[n_sel ..) = cates[sel], which removes one of the two indirections of items[sel[psrc]];
// feed_build_pos_kernel writes nothing when the status is set.
enum { FEED_SCAN_PARTS = 1024 };

__global__ void __launch_bounds__(256) feed_scan_pos_kernel(FeedArgs d, int* part) {
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = INT_MAX;
  __syncthreads();
  const int n_sel = (int)d.n_sel, per = (d.G - 1) * d.T, total = n_sel + (int)(d.n * per);
  const long p0 = d.h0 * per - n_sel;
  int bad = INT_MAX;
  // position of the first index that cannot be served: sel entries first, then the shard's psrc entries (ascending per
  // thread: the first hit is the thread's lowest)
  for (long i = blockIdx.x * 256 + threadIdx.x; i < total && bad == INT_MAX; i += gridDim.x * 256) {
    const bool ok = i < n_sel ? (unsigned)d.sel[i] < (unsigned long)d.N : (unsigned)d.src[p0 + i] < (unsigned)n_sel;
    if (!ok) bad = (int)i;
  }
  if (bad != INT_MAX) atomicMin(&s_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = s_bad;
}

__global__ void __launch_bounds__(1024) feed_check_pos_kernel(FeedArgs d, int* bt, const int* part, int nparts) {
  __shared__ int s_bad, s_cnt;
  if (threadIdx.x == 0) {
    s_bad = INT_MAX;
    s_cnt = 0;
  }
  __syncthreads();
  const int n_sel = (int)d.n_sel, per = (d.G - 1) * d.T;
  const long p0 = d.h0 * per;
  int bad = INT_MAX;
  for (int b = threadIdx.x; b < nparts; b += 1024) bad = min(bad, part[b]);
  if (bad != INT_MAX) atomicMin(&s_bad, bad);
  __syncthreads();
  bad = s_bad;
  if (bad != INT_MAX) {
    if (threadIdx.x == 0)
      feed_refuse(d.err, bad < n_sel ? 1 : 3, bad < n_sel ? bad : (int)p0 + (bad - n_sel),
                  bad < n_sel ? d.sel + bad : d.src + p0 + (bad - n_sel));
    return;
  }
  for (int i = threadIdx.x; i < n_sel; i += 1024) {
    const int line = d.sel[i];
    bt[i] = d.items[line];
    bt[n_sel + i] = d.cates[line];
  }
  feed_accept(d, &s_cnt);
}

template <typename W> struct feed_word;
template <> struct feed_word<unsigned> {
  static __device__ __forceinline__ unsigned get(unsigned w, int) { return w; }
  static __device__ __forceinline__ unsigned make(const unsigned* v) { return v[0]; }
};
template <> struct feed_word<feed_u32x4> {
  static __device__ __forceinline__ unsigned get(feed_u32x4 w, int k) { return k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w; }
  static __device__ __forceinline__ feed_u32x4 make(const unsigned* v) {
    feed_u32x4 w;
    w.x = v[0], w.y = v[1], w.z = v[2], w.w = v[3];
    return w;
  }
};

// Blocks [0, big_blocks): the four history arrays (feed_move_rows).  The next tgt_blocks: out_items / out_cates / out_labels
// [n G, T], a lane per output word W, consecutive lanes on consecutive steps of a row; a negative row reads its psrc row the
// same way.  The rest: users / seq_len.
template <typename W>
__global__ void __launch_bounds__(256) feed_build_pos_kernel(FeedArgs d, const int* __restrict__ bt, long nq, long nqt, int Tq,
                                                             int big_blocks, int tgt_blocks) {
  if (d.err[FEED_ERR_LAUNCH]) return;
  constexpr int WN = (int)(sizeof(W) / 4);
  const int G = d.G, T = d.T;
  if ((int)blockIdx.x < big_blocks) {
    feed_move_rows<W>(d, d, FeedTrainLine{d}, nq, Tq, big_blocks);
    return;
  }
  if ((int)blockIdx.x < big_blocks + tgt_blocks) {
    const int* __restrict__ bi = bt;
    const int* __restrict__ bc = bt + d.n_sel;
    const W* __restrict__ ps = (const W*)d.src;
    W* __restrict__ oi = (W*)d.out_items;
    W* __restrict__ oc = (W*)d.out_cates;
    W* __restrict__ ol = (W*)d.out_labels;
    for (long q = (long)(blockIdx.x - big_blocks) * 256 + threadIdx.x; q < nqt; q += (long)tgt_blocks * 256) {
      const long r = q / Tq;
      const int t0 = (int)(q - r * Tq) * WN;
      const long h = r / G;
      const int g = (int)(r - h * G);
      unsigned vi[WN], vc[WN], vl[WN];
      if (g == 0) {
        // the positive row: the line's history one step on, its target last
        const long base = (long)d.sel[d.h0 + h] * T;
#pragma unroll
        for (int k = 0; k < WN; ++k) {
          const int t = t0 + k;
          vi[k] = t == T - 1 ? (unsigned)bi[d.h0 + h] : (unsigned)d.item_history[base + t + 1];
          vc[k] = t == T - 1 ? (unsigned)bc[d.h0 + h] : (unsigned)d.item_cate_history[base + t + 1];
          vl[k] = __float_as_uint(1.0f);
        }
      } else {
        const W p = ps[((d.h0 + h) * (G - 1) + (g - 1)) * Tq + (t0 / WN)];
#pragma unroll
        for (int k = 0; k < WN; ++k) {
          const int j = (int)feed_word<W>::get(p, k);
          vi[k] = (unsigned)bi[j];
          vc[k] = (unsigned)bc[j];
          vl[k] = 0u;
        }
      }
      oi[q] = feed_word<W>::make(vi);
      oc[q] = feed_word<W>::make(vc);
      ol[q] = feed_word<W>::make(vl);
    }
    return;
  }
  const long R = d.expanded ? d.n * G : d.n;
  const long stride = (long)(gridDim.x - big_blocks - tgt_blocks) * 256;
  for (long b = (long)(blockIdx.x - big_blocks - tgt_blocks) * 256 + threadIdx.x; b < R; b += stride) {
    const int own = d.sel[d.h0 + (d.expanded ? b / G : b)];
    d.out_users[b] = d.users[own];
    d.out_seq_len[b] = d.lens[own];
  }
}

extern "C" long clsr_feed_build_pos_scratch_ints(long n_sel) { return n_sel < 0 ? 0 : 2 * n_sel + FEED_SCAN_PARTS; }

extern "C" int clsr_feed_build_pos_supported(long N, long n_sel, int T, int G) {
  return N >= 1 && N <= INT_MAX && n_sel >= 1 && T >= 1 && T <= clsr_feed_build_max_steps() && G >= 2 &&
         G <= clsr_feed_build_max_group() && n_sel <= INT_MAX / ((long)G * T) - 1;
}

extern "C" int clsr_feed_build_pos(const void* const* cols_host, long N, const int* sel, long n_sel, const int* psrc, long h0,
                                   long n, int T, int G, int expanded, int thr, void* const* outs_host, int* scratch, int* err,
                                   void* stream) {
  CLSR_CHECK_ARG(scratch);
  FeedArgs d;
  const int rc = feed_train_args(d, cols_host, N, sel, n_sel, psrc, h0, n, T, G, expanded, thr, outs_host, err,
                                 clsr_feed_build_pos_supported(N, n_sel, T, G));
  if (rc != CLSR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  int* part = scratch + 2 * d.n_sel;
  long scan = (d.n_sel + d.n * (d.G - 1) * d.T + 2047) / 2048;      // eight positions a thread
  if (scan > FEED_SCAN_PARTS) scan = FEED_SCAN_PARTS;
  hipLaunchKernelGGL(feed_scan_pos_kernel, dim3((int)scan), dim3(256), 0, st, d, part);
  CLSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(feed_check_pos_kernel, dim3(1), dim3(1024), 0, st, d, scratch, (const int*)part, (int)scan);
  CLSR_CHECK_LAUNCH();
  const bool wide = feed_wide_rows(d.T, d, d) && feed_wide(d.T, {d.src, d.out_items, d.out_cates, d.out_labels});
  const int Tq = wide ? d.T / 4 : d.T;
  const long R = d.n * (d.expanded ? d.G : 1), nq = R * Tq, nqt = d.n * d.G * Tq;
  const int big = feed_blocks(nq, FEED_BIG_BLOCKS), tgt = feed_blocks(nqt, FEED_BIG_BLOCKS),
            small = feed_blocks(R, FEED_SMALL_BLOCKS);
  FEED_LAUNCH(feed_build_pos_kernel, wide, big + tgt + small, st, d, (const int*)scratch, nq, nqt, Tq, big, tgt);
  return CLSR_OK;
}

extern "C" int clsr_feed_clear_error(int* err, void* stream) {
  CLSR_CHECK_ARG(err);
  CLSR_HIP(hipMemsetAsync(err, 0, 4 * sizeof(int), (hipStream_t)stream));
  return CLSR_OK;
}

extern "C" int clsr_feed_error(const int* err, void* stream) {
  CLSR_CHECK_ARG(err);
  int e[4] = {0, 0, 0, 0};
  CLSR_HIP(hipStreamSynchronize((hipStream_t)stream));
  CLSR_HIP(hipMemcpy(e, err, sizeof(e), hipMemcpyDeviceToHost));
  if (e[FEED_ERR_CODE] == 0) return CLSR_OK;
  if (e[FEED_ERR_CODE] == 1)
    clsr_set_error("clsr_feed_build: sel[%d] = %d is not a line of the resident file", e[FEED_ERR_INDEX], e[FEED_ERR_VALUE]);
  else if (e[FEED_ERR_CODE] == 2)
    clsr_set_error("clsr_feed_build: src[%d] = %d is not a line of the batch", e[FEED_ERR_INDEX], e[FEED_ERR_VALUE]);
  else
    clsr_set_error("clsr_feed_build_pos: psrc[%d] = %d is not a line of the batch", e[FEED_ERR_INDEX], e[FEED_ERR_VALUE]);
  return CLSR_EINVAL;
}

// ---------------------------------------------------------------------------------------------------------------------
// Evaluation feeds from a resident column store (clsr_amd/resident.py, ResidentEvalStore).
//
// An evaluation pass yields the file lines keep[0 .. n_keep) in order (every entry checked against [0, N) on the host
// before keep is uploaded), batch_size lines a batch; lines of one positive share a history.  clsr_feed_same_rows marks,
// once per (file, keep), every line whose history-level columns equal those of the line before it; the host turns the
// marks into chunks (k0, n, g) and clsr_feed_build_eval writes the arena CLSRNet.upload(feed, False) would have filled for
// a chunk: history-level tensors from every g-th line, line-level tensors from every line.  One launch each.
struct FeedEvalArgs : FeedCols, FeedOuts {
  const int* keep;
  long k0, n;
  int g, T, thr;
};

// the user id as the host path carries it: through the float32 placeholder of the reference and back
__device__ __forceinline__ int feed_user_id(int id) { return (int)(float)id; }

// words of the integer columns differ by bits, words of the float columns as numpy's == has it (-0.0 equals 0.0, a NaN
// equals nothing)
__device__ __forceinline__ bool feed_differ(unsigned a, unsigned b, bool fp) {
  return fp ? !(__uint_as_float(a) == __uint_as_float(b)) : a != b;
}
__device__ __forceinline__ bool feed_differ(feed_u32x4 a, feed_u32x4 b, bool fp) {
  return feed_differ(a.x, b.x, fp) | feed_differ(a.y, b.y, fp) | feed_differ(a.z, b.z, fp) | feed_differ(a.w, b.w, fp);
}

// A wave per pair of lines (keep[i - 1], keep[i]); lanes on consecutive words, the four [N, T] columns together; the pair
// is left at the first 64-word slice that holds a difference.  i, and so every branch below, is uniform in the wave.
template <typename W>
__global__ void __launch_bounds__(256) feed_same_rows_kernel(FeedEvalArgs d, long n_keep, int Tq, unsigned char* flags) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwave = (long)gridDim.x * 4;
  if (wave == 0 && lane == 0) flags[0] = 0;
  const W* __restrict__ c0 = (const W*)d.item_history;
  const W* __restrict__ c1 = (const W*)d.item_cate_history;
  const W* __restrict__ c2 = (const W*)d.time_from_first_action;
  const W* __restrict__ c3 = (const W*)d.time_to_now;
  for (long i = 1 + wave; i < n_keep; i += nwave) {
    const long a = d.keep[i], b = d.keep[i - 1];
    bool diff = feed_user_id(d.users[a]) != feed_user_id(d.users[b]) || d.lens[a] != d.lens[b];
    for (int s = 0; s < Tq && !diff; s += 64) {
      const int c = s + lane;
      bool mine = false;
      if (c < Tq) {
        const long pa = a * Tq + c, pb = b * Tq + c;
        const W x0 = c0[pa], x1 = c1[pa], x2 = c2[pa], x3 = c3[pa];
        const W y0 = c0[pb], y1 = c1[pb], y2 = c2[pb], y3 = c3[pb];
        mine = feed_differ(x0, y0, false) | feed_differ(x1, y1, false) | feed_differ(x2, y2, true) | feed_differ(x3, y3, true);
      }
      diff = __any(mine) != 0;
    }
    if (lane == 0) flags[i] = diff ? 0 : 1;
  }
}

// Blocks [0, big_blocks): the four [n / g, T] arrays, a lane per word.  The next blocks: the line-level arrays and, from
// the first line of every group, users / seq_len.  The last block counts the histories longer than thr (an integer) and
// writes denom.
template <typename W>
__global__ void __launch_bounds__(256) feed_build_eval_kernel(FeedEvalArgs d, long nq, int Tq, int big_blocks) {
  const int g = d.g;
  const int* __restrict__ keep = d.keep + d.k0;
  if ((int)blockIdx.x < big_blocks) {
    feed_move_rows<W>(d, d, FeedEvalLine{keep, g}, nq, Tq, big_blocks);
    return;
  }
  const int small_blocks = (int)gridDim.x - big_blocks - 1;
  if ((int)blockIdx.x < big_blocks + small_blocks) {
    for (long b = (long)(blockIdx.x - big_blocks) * 256 + threadIdx.x; b < d.n; b += (long)small_blocks * 256) {
      const int line = keep[b];
      d.out_items[b] = d.items[line];
      d.out_cates[b] = d.cates[line];
      d.out_labels[b] = d.labels[line];
      const int user = feed_user_id(d.users[line]);
      if (d.out_users_rows) d.out_users_rows[b] = user;
      const long h = b / g;
      if (b == h * g) {
        d.out_users[h] = user;
        d.out_seq_len[h] = d.lens[line];
      }
    }
    return;
  }
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  int cnt = 0;
  for (long h = threadIdx.x; h < d.n / g; h += 256) cnt += d.lens[keep[h * g]] > d.thr ? 1 : 0;
  if (cnt) atomicAdd(&s_cnt, cnt);          // integer sum: the value does not depend on the order
  __syncthreads();
  if (threadIdx.x == 0) d.out_denom[0] = (float)((long)s_cnt * g);
}

extern "C" int clsr_feed_build_eval_supported(long N, long n_keep, long k0, long n, int g, int T) {
  return N >= 1 && N <= INT_MAX && n_keep >= 1 && n_keep <= INT_MAX && T >= 1 && T <= clsr_feed_build_max_steps() &&
         g >= 1 && n >= 1 && n % g == 0 && k0 >= 0 && k0 <= n_keep && n <= n_keep - k0 && (n / g) * (long)T <= INT_MAX;
}

extern "C" int clsr_feed_same_rows(const void* const* cols_host, long N, const int* keep, long n_keep, int T,
                                   unsigned char* flags, void* stream) {
  CLSR_CHECK_ARG(keep && flags);
  FeedEvalArgs d = {};
  CLSR_CHECK_ARG(feed_cols(d, cols_host, 6));
  d.keep = keep;
  d.T = T;
  CLSR_CHECK_ARG(N >= 1 && N <= INT_MAX && n_keep >= 1 && n_keep <= INT_MAX && T >= 1 && T <= clsr_feed_build_max_steps());
  const bool wide = feed_wide(T, {d.item_history, d.item_cate_history, d.time_from_first_action, d.time_to_now});
  const int Tq = wide ? T / 4 : T;
  long blocks = (n_keep + 3) / 4;            // four waves, four pairs a workgroup
  if (blocks > 8192) blocks = 8192;
  FEED_LAUNCH(feed_same_rows_kernel, wide, (int)blocks, (hipStream_t)stream, d, n_keep, Tq, flags);
  return CLSR_OK;
}

extern "C" int clsr_feed_build_eval(const void* const* cols_host, long N, const int* keep, long n_keep, long k0, long n,
                                    int g, int T, int thr, void* const* outs_host, void* stream) {
  CLSR_CHECK_ARG(keep);
  FeedEvalArgs d = {};
  CLSR_CHECK_ARG(feed_cols(d, cols_host, 9));
  CLSR_CHECK_ARG(feed_outs(d, outs_host, true));
  d.keep = keep;
  d.k0 = k0, d.n = n, d.g = g, d.T = T, d.thr = thr;
  CLSR_CHECK_ARG(d.out_users_rows || g == 1);
  CLSR_CHECK_ARG(clsr_feed_build_eval_supported(N, n_keep, k0, n, g, T));
  const bool wide = feed_wide_rows(T, d, d);
  const int Tq = wide ? T / 4 : T;
  const long nq = (n / g) * Tq;
  const int big = feed_blocks(nq, FEED_BIG_BLOCKS), small = feed_blocks(n, FEED_SMALL_BLOCKS);
  FEED_LAUNCH(feed_build_eval_kernel, wide, big + small + 1, (hipStream_t)stream, d, nq, Tq, big);
  return CLSR_OK;
}
