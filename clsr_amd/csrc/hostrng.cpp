// Host-side replay of CPython's `random` module (MT19937) for the input pipeline (no GPU work here).
//
// The reference iterator shuffles the cached list of parsed train lines with random.shuffle on every pass and draws
// the in-batch negatives with random.randint (io/sequential_iterator.py:249-261, 612-634).  To keep the batch
// stream bit-identical while leaving the interpreter out of a 1M-element shuffle, these entry points continue the
// generator from a state exported by random.getstate() and hand the advanced state back for random.setstate().
//   getrandbits(k <= 32) == genrand_uint32() >> (32 - k);  _randbelow(n): k = n.bit_length(), redraw while r >= n;
//   shuffle(x): for i = len-1 .. 1: j = _randbelow(i + 1); swap(x[i], x[j])        (CPython 3.10 Lib/random.py)
#include "common.h"
#include "clsr_hip.h"

namespace {
struct MT {
  uint32_t* mt;
  int idx;
  inline void twist() {   // the next block of 624 words
    static const uint32_t mag01[2] = {0u, 0x9908b0dfu};
    int kk = 0;
    uint32_t y;
    for (; kk < 624 - 397; ++kk) {
      y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
      mt[kk] = mt[kk + 397] ^ (y >> 1) ^ mag01[y & 1u];
    }
    for (; kk < 623; ++kk) {
      y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
      mt[kk] = mt[kk + (397 - 624)] ^ (y >> 1) ^ mag01[y & 1u];
    }
    y = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
    mt[623] = mt[396] ^ (y >> 1) ^ mag01[y & 1u];
    idx = 0;
  }
  static inline uint32_t temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
  }
  inline uint32_t next() {
    if (idx >= 624) twist();
    return temper(mt[idx++]);
  }
  inline uint32_t below(uint32_t n) {  // random._randbelow_with_getrandbits, n >= 1
    int k = 0;
    for (uint32_t v = n; v; v >>= 1) ++k;
    uint32_t r = next() >> (32 - k);
    while (r >= n) r = next() >> (32 - k);
    return r;
  }
};
}  // namespace

// perm (n entries) is shuffled in place exactly like random.shuffle(list) would; key[624] / *pos = MT state.
extern "C" int clsr_host_mt_shuffle(unsigned* key, int* pos, long* perm, long n) {
  CLSR_CHECK_ARG(key && pos && perm && n >= 0 && *pos >= 0 && *pos <= 624);
  CLSR_CHECK_SUPPORTED(n < (1L << 31));
  MT g{key, *pos};
  for (long i = n - 1; i >= 1; --i) {
    const long j = g.below((uint32_t)(i + 1));
    const long t = perm[i];
    perm[i] = perm[j];
    perm[j] = t;
  }
  *pos = g.idx;
  return CLSR_OK;
}

// In-batch negative sampling of one training batch (sequential_iterator.py:612-634): for every line i, ngs draws
// j = randint(0, n-1), redrawn while items[j] == items[i]; src[i*(ngs+1)] = i, then the accepted j's.
extern "C" int clsr_host_mt_sample_negatives(unsigned* key, int* pos, const long* items, long n, int ngs,
                                             long* src) {
  CLSR_CHECK_ARG(key && pos && items && src && n >= 2 && ngs >= 1 && *pos >= 0 && *pos <= 624);
  CLSR_CHECK_SUPPORTED(n < (1L << 31));
  MT g{key, *pos};
  for (long i = 0; i < n; ++i) {
    long* row = src + i * (ngs + 1);
    row[0] = i;
    const long own = items[i];
    int count = 0;
    long guard = 0;
    while (count < ngs) {
      const long j = g.below((uint32_t)n);
      if (items[j] == own) {
        if (++guard > (1L << 24)) {   // a batch whose items are all equal would never terminate in the reference
          clsr_set_error("clsr_host_mt_sample_negatives: every draw equals the positive item of line %ld", i);
          return CLSR_EINVAL;
        }
        continue;
      }
      row[++count] = j;
    }
  }
  *pos = g.idx;
  return CLSR_OK;
}

// Per-position negative sampling of one NextItNet training batch (io/nextitnet_iterator.py; NextItNetIterator._convert_data):
// for line i, negative g = 1 .. ngs, step t = 0 .. T - 1, in that order, j = randint(0, n - 1), redrawn while items[j] ==
// pos_rows[i * T + t]; psrc[(i * ngs + g - 1) * T + t] = the accepted j.  pos_rows [n, T]: the positive row of every line as
// the literal path builds it (the left-padded history one step on, the target last, padding zeros included).
// A position no line of the batch can serve (every items[j] equals it) would never end in the reference: the batch is
// looked over BEFORE the first draw, and the call returns CLSR_HOST_MT_NO_DRAW with key / *pos / psrc untouched.
extern "C" int clsr_host_mt_sample_negatives_pos(unsigned* key, int* pos, const int* items, const int* pos_rows, long n,
                                                 int ngs, int T, int* psrc) {
  CLSR_CHECK_ARG(key && pos && items && pos_rows && psrc && n >= 2 && ngs >= 1 && T >= 1 && *pos >= 0 && *pos <= 624);
  CLSR_CHECK_SUPPORTED(n < (1L << 31));
  bool one_item = true;
  for (long j = 1; j < n && one_item; ++j) one_item = items[j] == items[0];
  if (one_item)       // (two different items: whatever a position holds, one of them differs from it)
    for (long q = 0; q < n * T; ++q)
      if (pos_rows[q] == items[0]) return CLSR_HOST_MT_NO_DRAW;
  MT g{key, *pos};
  const uint32_t un = (uint32_t)n;
  int k = 0;
  for (uint32_t v = un; v; v >>= 1) ++k;
  const int shift = 32 - k;
  // _randbelow drops every output >= n (half of them when n is a power of two): a data-dependent branch per output would
  // be mispredicted at that rate.  The rest of the current block is tempered at once and its candidates < n compacted
  // without a branch, each with the place of its word in the block; the draws then walk the candidates, where the only
  // branch left is the rare hit on the positive.  The state handed back is the word after the last candidate USED: the
  // outputs dropped behind it belong to a randint call that has not been made.
  uint32_t cand[624];
  int at[624], nc = 0, ci = 0;
  for (long i = 0; i < n; ++i) {
    const int* own = pos_rows + i * T;
    int* out = psrc + i * (long)ngs * T;
    for (int c = 0; c < ngs; ++c, out += T)
      for (int t = 0; t < T; ++t) {
        const int p = own[t];
        uint32_t j;
        do {
          while (ci == nc) {
            if (g.idx >= 624) g.twist();
            nc = ci = 0;
            for (int r = g.idx; r < 624; ++r) {
              const uint32_t v = MT::temper(g.mt[r]) >> shift;
              cand[nc] = v;
              at[nc] = r;
              nc += v < un ? 1 : 0;
            }
            g.idx = 624;
          }
          j = cand[ci++];
        } while (items[j] == p);
        out[t] = (int)j;
      }
  }
  g.idx = at[ci - 1] + 1;
  *pos = g.idx;
  return CLSR_OK;
}
