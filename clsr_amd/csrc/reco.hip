// recommend_k_items on the device (clsr_amd/recommend.py): everything around the scoring kernels.
//
// A request batch of Hn histories is scored against the catalogue in chunks of g candidates: reco_fill_kernel writes the
// chunk's ids into the items / cates tensors of the compact scoring feed (row h * g + j = candidate c0 + j, id 0 past the
// catalogue's end), the existing forward pass gives logit [Hn * g], and reco_topk_kernel merges the chunk's first n_valid
// candidates of every history into its running list of the K best.
//
// The order is total: a before b iff score_a > score_b, or the scores compare equal (IEEE: -0.0 ties with +0.0) and
// item_a < item_b.  It is carried by ONE 64-bit key per candidate, larger = better:
//   high word: the score's bits (-0.0 canonicalised to +0.0 first) mapped monotonically to unsigned,
//   low word:  ~item, so that the smaller id of two equal scores has the larger key.
// An empty slot is (-inf, -1): high word of -inf, low word ~(-1) = 0 -- below every finite candidate, and it decodes to
// itself, so empty slots need no flag.  Keys of distinct candidates are distinct, so the K largest keys of a set do not
// depend on how the set was cut into chunks, on the order inside a chunk or on the launch geometry.
//
// One workgroup of 256 threads per history.  LDS: 4096 keys (32 KB: the running list in front, the chunk's survivors behind
// it), the history row (T <= 256 ids, 1 KB), four wave counts.  A candidate survives when its key beats the list's K-th
// entry (nothing else can enter) and, with remove_seen, when its id is not one of the T ids of the history row (padding is
// id 0, never a candidate: no lengths needed).  Survivors are compacted behind the list with wave ballots and per-wave
// counts (no atomics anywhere); list + survivors, padded with empty keys to a power of two P, are sorted by a bitonic
// network in LDS and the first K keys are decoded into best_score / best_item.  After the first chunks few candidates beat
// the K-th entry, so P is usually the smallest power of two above K.
#include "clsr_hip.h"
#include "common.h"

#include <limits.h>

typedef unsigned long long reco_key;

enum { RECO_KEYS = 4096, RECO_MAX_K = 256, RECO_MAX_T = 256, RECO_MAX_CHUNK = RECO_KEYS - RECO_MAX_K, RECO_FILL_BLOCKS = 4096 };

#define RECO_EMPTY ((reco_key)0x007FFFFFu << 32)      // (-inf, -1)

__device__ __forceinline__ reco_key reco_encode(float score, int item) {
  unsigned b = __float_as_uint(score);
  if (b == 0x80000000u) b = 0u;                        // -0.0 -> +0.0: the two zeros tie
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((reco_key)b << 32) | (unsigned)~item;
}
__device__ __forceinline__ void reco_decode(reco_key k, float& score, int& item) {
  const unsigned o = (unsigned)(k >> 32);
  score = __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
  item = (int)~(unsigned)k;
}

__global__ void __launch_bounds__(256) reco_fill_kernel(const int* __restrict__ cand_items, const int* __restrict__ cand_cates,
                                                        long M, long c0, int g, long total, int* __restrict__ items,
                                                        int* __restrict__ cates) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long c = c0 + (i % g);
    const bool in = c < M;
    items[i] = in ? cand_items[c] : 0;
    cates[i] = in ? cand_cates[c] : 0;
  }
}

__global__ void __launch_bounds__(256) reco_topk_kernel(const float* __restrict__ logit, const int* __restrict__ items, int g,
                                                        int n_valid, const int* __restrict__ hist_items, long hist_row_stride,
                                                        int T, int remove_seen, int K, float* __restrict__ best_score,
                                                        int* __restrict__ best_item, int first) {
  __shared__ reco_key keys[RECO_KEYS];
  __shared__ int seen[RECO_MAX_T];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long h = blockIdx.x;
  float* bs = best_score + h * K;
  int* bi = best_item + h * K;
  for (int k = tid; k < K; k += 256) keys[k] = first ? RECO_EMPTY : reco_encode(bs[k], bi[k]);
  if (remove_seen)
    for (int t = tid; t < T; t += 256) seen[t] = hist_items[h * hist_row_stride + t];
  __syncthreads();
  const reco_key kth = keys[K - 1];          // the list is sorted: its last entry is the one to beat
  const float* lg = logit + h * g;
  const int* it = items + h * g;
  int n = K;                                  // keys in LDS so far (uniform in the workgroup)
  for (int j0 = 0; j0 < n_valid; j0 += 256) {
    const int j = j0 + tid;
    reco_key key = RECO_EMPTY;
    bool keep = false;
    if (j < n_valid) {
      const int id = it[j];
      key = reco_encode(lg[j], id);
      keep = key > kth;
      if (keep && remove_seen)
        for (int t = 0; t < T; ++t) keep &= seen[t] != id;      // (every lane reads the same word: a broadcast)
    }
    const unsigned long long ballot = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(ballot);
    __syncthreads();
    int base = n;
    for (int w = 0; w < wave; ++w) base += wcnt[w];
    if (keep) keys[base + __popcll(ballot & ((1ull << lane) - 1ull))] = key;      // base + rank < K + n_valid <= RECO_KEYS
    n += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  if (n == K && !first) return;               // nothing entered: the list stands as it is (uniform branch)
  int P = 2;
  while (P < n) P <<= 1;                      // <= RECO_KEYS: n <= K + n_valid <= 4096
  for (int i = n + tid; i < P; i += 256) keys[i] = RECO_EMPTY;
  __syncthreads();
  // bitonic network, descending; comparator c of a stage with distance d works on i = c with a zero inserted at bit d
  for (int k = 2; k <= P; k <<= 1) {
    for (int d = k >> 1; d > 0; d >>= 1) {
      for (int c = tid; c < (P >> 1); c += 256) {
        const int i = ((c & ~(d - 1)) << 1) | (c & (d - 1)), l = i | d;
        const reco_key a = keys[i], b = keys[l];
        if (((i & k) == 0) ? a < b : a > b) {
          keys[i] = b;
          keys[l] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int k = tid; k < K; k += 256) {
    float s;
    int id;
    reco_decode(keys[k], s, id);
    bs[k] = s;
    bi[k] = id;
  }
}

// ---- rank of one target against the catalogue (clsr_amd/recommend.py: rank_targets).  The rank of an item is a count, not a
// sort: column 0 of every group holds the request's target (reco_fill_ranked_kernel), re-scored with every chunk by the same
// launch to the same bits, so the count needs no state about the target, no pre-pass and no order among the chunks.
// reco_rank_kernel: grid (Hn, slabs), a workgroup per request and slab of RECO_RANK_SLAB candidate columns, a column per
// thread.  A column 1 .. n_valid counts when its id is not the target's, its key beats the target's and, with remove_seen,
// its id is none of the T ids of the history row (staged in LDS, read as a broadcast).  Ballot + popcount per wave, four wave
// counts summed by thread 0, which owns partial[h, slab]: first overwrites it, otherwise it is added to.  No atomics.
enum { RECO_RANK_SLAB = 256 };

__global__ void __launch_bounds__(256) reco_fill_ranked_kernel(const int* __restrict__ cand_items, const int* __restrict__ cand_cates,
                                                               long M, long c0, int g, const int* __restrict__ target_items,
                                                               const int* __restrict__ target_cates, long total,
                                                               int* __restrict__ items, int* __restrict__ cates) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long h = i / g;
    const int j = (int)(i - h * g);
    const long c = c0 + j - 1;
    const bool in = j > 0 && c < M;
    items[i] = j == 0 ? target_items[h] : in ? cand_items[c] : 0;
    cates[i] = j == 0 ? target_cates[h] : in ? cand_cates[c] : 0;
  }
}

__global__ void __launch_bounds__(256) reco_rank_kernel(const float* __restrict__ logit, const int* __restrict__ items, int g,
                                                        int n_valid, const int* __restrict__ hist_items, long hist_row_stride,
                                                        int T, int remove_seen, int* __restrict__ partial,
                                                        float* __restrict__ target_score, int first) {
  __shared__ int seen[RECO_MAX_T];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long h = blockIdx.x;
  const int slab = blockIdx.y;
  int* slot = partial + h * gridDim.y + slab;
  if (slab * RECO_RANK_SLAB >= n_valid) {     // a slab past the ragged chunk's end (uniform branch): nothing to read
    if (first && tid == 0) *slot = 0;
    return;
  }
  if (remove_seen)
    for (int t = tid; t < T; t += 256) seen[t] = hist_items[h * hist_row_stride + t];
  const float* lg = logit + h * g;
  const int* it = items + h * g;
  const float ts = lg[0];
  const int target = it[0];
  const reco_key tkey = reco_encode(ts, target);
  __syncthreads();
  const int j = 1 + slab * RECO_RANK_SLAB + tid;      // <= g - 1 where it is read: n_valid <= g - 1
  bool beats = false;
  if (j <= n_valid) {
    const int id = it[j];
    beats = id != target && reco_encode(lg[j], id) > tkey;
    if (beats && remove_seen)
      for (int t = 0; t < T; ++t) beats &= seen[t] != id;       // (every lane reads the same word: a broadcast)
  }
  const unsigned long long ballot = __ballot(beats);
  if (lane == 0) wcnt[wave] = __popcll(ballot);
  __syncthreads();
  if (tid == 0) {
    const int n = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    *slot = first ? n : *slot + n;
    if (first && slab == 0) target_score[h] = ts;
  }
}

extern "C" int clsr_reco_max_chunk(void) { return RECO_MAX_CHUNK; }
extern "C" int clsr_reco_max_k(void) { return RECO_MAX_K; }

extern "C" int clsr_reco_topk_supported(long Hn, int g, int T, int K) {
  return Hn >= 1 && Hn <= INT_MAX && g >= 1 && g <= RECO_MAX_CHUNK && T >= 1 && T <= RECO_MAX_T && K >= 1 && K <= RECO_MAX_K &&
         Hn * (long)g <= INT_MAX;
}

extern "C" int clsr_reco_fill_candidates(const int* cand_items, const int* cand_cates, long M, long c0, int g, long Hn,
                                         int* items, int* cates, void* stream) {
  CLSR_CHECK_ARG(cand_items && cand_cates && items && cates);
  CLSR_CHECK_ARG(M >= 1 && c0 >= 0 && c0 < M && g >= 1 && Hn >= 1);
  CLSR_CHECK_SUPPORTED(M <= INT_MAX && Hn * (long)g <= INT_MAX);
  const long total = Hn * g;
  long blocks = (total + 255) / 256;
  if (blocks > RECO_FILL_BLOCKS) blocks = RECO_FILL_BLOCKS;
  hipLaunchKernelGGL(reco_fill_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, cand_items, cand_cates, M, c0, g,
                     total, items, cates);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_reco_topk_merge(const float* logit, const int* items, long Hn, int g, int n_valid, const int* hist_items,
                                    long hist_row_stride, int T, int remove_seen, int K, float* best_score, int* best_item,
                                    int first, void* stream) {
  CLSR_CHECK_ARG(logit && items && best_score && best_item);
  CLSR_CHECK_SUPPORTED(clsr_reco_topk_supported(Hn, g, T, K));
  CLSR_CHECK_ARG(n_valid >= 1 && n_valid <= g);
  CLSR_CHECK_ARG(!remove_seen || (hist_items && hist_row_stride >= T));
  hipLaunchKernelGGL(reco_topk_kernel, dim3((int)Hn), dim3(256), 0, (hipStream_t)stream, logit, items, g, n_valid, hist_items,
                     hist_row_stride, T, remove_seen ? 1 : 0, K, best_score, best_item, first ? 1 : 0);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_reco_rank_slab(void) { return RECO_RANK_SLAB; }

extern "C" int clsr_reco_rank_supported(long Hn, int g, int T) {
  if (!(Hn >= 1 && Hn <= INT_MAX && g >= 2 && T >= 1 && T <= RECO_MAX_T && Hn * (long)g <= INT_MAX)) return 0;
  const long slabs = ((long)g - 1 + RECO_RANK_SLAB - 1) / RECO_RANK_SLAB;
  return slabs <= 65535 && Hn * slabs <= INT_MAX;
}

extern "C" int clsr_reco_fill_ranked(const int* cand_items, const int* cand_cates, long M, long c0, int g, const int* target_items,
                                     const int* target_cates, long Hn, int* items, int* cates, void* stream) {
  CLSR_CHECK_ARG(cand_items && cand_cates && target_items && target_cates && items && cates);
  CLSR_CHECK_ARG(M >= 1 && c0 >= 0 && c0 < M && g >= 2 && Hn >= 1);
  CLSR_CHECK_SUPPORTED(M <= INT_MAX && Hn * (long)g <= INT_MAX);
  const long total = Hn * g;
  long blocks = (total + 255) / 256;
  if (blocks > RECO_FILL_BLOCKS) blocks = RECO_FILL_BLOCKS;
  hipLaunchKernelGGL(reco_fill_ranked_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, cand_items, cand_cates, M, c0,
                     g, target_items, target_cates, total, items, cates);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_reco_rank_count(const float* logit, const int* items, long Hn, int g, int n_valid, const int* hist_items,
                                    long hist_row_stride, int T, int remove_seen, int* partial, float* target_score, int first,
                                    void* stream) {
  CLSR_CHECK_ARG(logit && items && partial && (!first || target_score));
  CLSR_CHECK_SUPPORTED(clsr_reco_rank_supported(Hn, g, T));
  CLSR_CHECK_ARG(n_valid >= 1 && n_valid <= g - 1);
  CLSR_CHECK_ARG(!remove_seen || (hist_items && hist_row_stride >= T));
  const int slabs = (g - 1 + RECO_RANK_SLAB - 1) / RECO_RANK_SLAB;
  hipLaunchKernelGGL(reco_rank_kernel, dim3((int)Hn, slabs), dim3(256), 0, (hipStream_t)stream, logit, items, g, n_valid,
                     hist_items, hist_row_stride, T, remove_seen ? 1 : 0, partial, target_score, first ? 1 : 0);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}
