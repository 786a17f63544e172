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

typedef unsigned feed_u32x4 __attribute__((ext_vector_type(4)));

// the arguments of one call as the kernels take them (by value)
struct FeedArgs {
  const int* item_history; const int* item_cate_history; const float* time_from_first_action; const float* time_to_now;
  const int* lens; const int* users; const int* items; const int* cates;
  const int* sel; const int* src;
  int* out_users; int* out_items; int* out_cates; int* out_item_history; int* out_item_cate_history;
  float* out_time_from_first_action; float* out_time_to_now; float* out_labels; int* out_seq_len; float* out_denom;
  int* err;
  long N, n_sel, h0, n;
  int T, G, expanded, thr;
};

enum { FEED_ERR_CODE = 0, FEED_ERR_INDEX = 1, FEED_ERR_VALUE = 2, FEED_ERR_LAUNCH = 3 };

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
    if (threadIdx.x == 0) {
      if (d.err[FEED_ERR_CODE] == 0) {      // sticky: the first failure stays until clsr_feed_clear_error
        d.err[FEED_ERR_CODE] = bad < n_sel ? 1 : 2;
        d.err[FEED_ERR_INDEX] = bad < n_sel ? bad : bad - n_sel;
        d.err[FEED_ERR_VALUE] = bad < n_sel ? d.sel[bad] : d.src[row0 + (bad - n_sel)];
      }
      d.err[FEED_ERR_LAUNCH] = 1;
    }
    return;
  }
  int cnt = 0;
  for (int i = threadIdx.x; i < (int)d.n; i += 1024) cnt += d.lens[d.sel[d.h0 + i]] > d.thr ? 1 : 0;
  if (cnt) atomicAdd(&s_cnt, cnt);          // integer sum: the value does not depend on the order
  __syncthreads();
  if (threadIdx.x == 0) {
    d.err[FEED_ERR_LAUNCH] = 0;
    d.out_denom[0] = (float)((long)s_cnt * d.G);
  }
}

// W: one 4-byte word or four per access.  A row of T words is contiguous on both sides and consecutive lanes walk
// consecutive words of it; the four history-level arrays move together (four independent loads in flight per lane).
template <typename W>
__global__ void __launch_bounds__(256) feed_build_kernel(FeedArgs d, long nq, int Tq, int big_blocks) {
  if (d.err[FEED_ERR_LAUNCH]) return;
  const int G = d.G;
  if ((int)blockIdx.x < big_blocks) {
    const W* __restrict__ c0 = (const W*)d.item_history;
    const W* __restrict__ c1 = (const W*)d.item_cate_history;
    const W* __restrict__ c2 = (const W*)d.time_from_first_action;
    const W* __restrict__ c3 = (const W*)d.time_to_now;
    W* __restrict__ o0 = (W*)d.out_item_history;
    W* __restrict__ o1 = (W*)d.out_item_cate_history;
    W* __restrict__ o2 = (W*)d.out_time_from_first_action;
    W* __restrict__ o3 = (W*)d.out_time_to_now;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)big_blocks * 256) {
      const long r = q / Tq;
      const int c = (int)(q - r * Tq);
      const long line = d.sel[d.h0 + (d.expanded ? r / G : r)];
      const long s = line * Tq + c;
      const W v0 = c0[s], v1 = c1[s], v2 = c2[s], v3 = c3[s];
      o0[q] = v0;
      o1[q] = v1;
      o2[q] = v2;
      o3[q] = v3;
    }
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

extern "C" int clsr_feed_build(const void* const* cols_host, long N, const int* sel, long n_sel, const int* src, long h0,
                               long n, int T, int G, int expanded, int thr, void* const* outs_host, int* err, void* stream) {
  CLSR_CHECK_ARG(cols_host && outs_host);
  FeedArgs d;
  d.item_history = (const int*)cols_host[0];
  d.item_cate_history = (const int*)cols_host[1];
  d.time_from_first_action = (const float*)cols_host[2];
  d.time_to_now = (const float*)cols_host[3];
  d.lens = (const int*)cols_host[4];
  d.users = (const int*)cols_host[5];
  d.items = (const int*)cols_host[6];
  d.cates = (const int*)cols_host[7];
  d.sel = sel;
  d.src = src;
  d.out_users = (int*)outs_host[0];
  d.out_items = (int*)outs_host[1];
  d.out_cates = (int*)outs_host[2];
  d.out_item_history = (int*)outs_host[3];
  d.out_item_cate_history = (int*)outs_host[4];
  d.out_time_from_first_action = (float*)outs_host[5];
  d.out_time_to_now = (float*)outs_host[6];
  d.out_labels = (float*)outs_host[7];
  d.out_seq_len = (int*)outs_host[8];
  d.out_denom = (float*)outs_host[9];
  d.err = err;
  d.N = N, d.n_sel = n_sel, d.h0 = h0, d.n = n;
  d.T = T, d.G = G, d.expanded = expanded, d.thr = thr;
  CLSR_CHECK_ARG(d.item_history && d.item_cate_history && d.time_from_first_action && d.time_to_now);
  CLSR_CHECK_ARG(d.lens && d.users && d.items && d.cates && d.sel && d.src && d.err);
  CLSR_CHECK_ARG(d.out_users && d.out_items && d.out_cates && d.out_item_history && d.out_item_cate_history);
  CLSR_CHECK_ARG(d.out_time_from_first_action && d.out_time_to_now && d.out_labels && d.out_seq_len && d.out_denom);
  CLSR_CHECK_SUPPORTED(clsr_feed_build_supported(d.N, d.n_sel, d.T, d.G));
  CLSR_CHECK_ARG(d.h0 >= 0 && d.n >= 1 && d.h0 + d.n <= d.n_sel);
  CLSR_CHECK_ARG(d.expanded == 0 || d.expanded == 1);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(feed_check_kernel, dim3(1), dim3(1024), 0, st, d);
  CLSR_CHECK_LAUNCH();
  // 16-byte accesses where every row starts on a 16-byte boundary on both sides (T = 50 does not)
  uintptr_t a = 0;
  for (const void* p : {(const void*)d.item_history, (const void*)d.item_cate_history, (const void*)d.time_from_first_action,
                        (const void*)d.time_to_now, (const void*)d.out_item_history, (const void*)d.out_item_cate_history,
                        (const void*)d.out_time_from_first_action, (const void*)d.out_time_to_now})
    a |= (uintptr_t)p;
  const bool wide = d.T % 4 == 0 && a % 16 == 0;
  const int Tq = wide ? d.T / 4 : d.T;
  const long nq = d.n * (d.expanded ? d.G : 1) * Tq;
  long big = (nq + 255) / 256, small = (d.n * d.G + 255) / 256;
  if (big > 16384) big = 16384;
  if (small > 1024) small = 1024;
  if (wide)
    hipLaunchKernelGGL(feed_build_kernel<feed_u32x4>, dim3((int)(big + small)), dim3(256), 0, st, d, nq, Tq, (int)big);
  else
    hipLaunchKernelGGL(feed_build_kernel<unsigned>, dim3((int)(big + small)), dim3(256), 0, st, d, nq, Tq, (int)big);
  CLSR_CHECK_LAUNCH();
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
  else
    clsr_set_error("clsr_feed_build: src[%d] = %d is not a line of the batch", e[FEED_ERR_INDEX], e[FEED_ERR_VALUE]);
  return CLSR_EINVAL;
}
