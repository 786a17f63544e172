// LGN (models/sequential/lgn.py): propagation of all N = Vu + Vi node rows through the normalised adjacency A_hat (CSR),
// a small dense layer fused behind the sparse product.  Per layer k and row r:
//
//   forward    S_k[r]     = sum_e values[e] E_k[indices[e]]                    e over the row's entries
//              E_{k+1}[r] = lrelu(S_k[r] . W_k + b_k)                          slope 0.2; the last layer also writes
//              F[r]       = (E_0[r] + E_1[r] + E_2[r]) / 3
//   backward   T[r]       = sum_e values^T[e] P_k[indices^T[e]]                the SAME gather, over the CSR of A_hat^T
//              out[r]     = (dF[r] / 3 + T[r] . W_k^T) * lrelu'(E_k[r])        = P_{k-1} (k = 0: no gate, out = dE_0)
//              dW_k       = S_k^T P_k,  db_k = column sums of P_k              over the workgroup's own rows
//
// with P_k = dE_{k+1} * lrelu'(E_{k+1}) (lrelu' read off the OUTPUT: 1 where it is positive, 0.2 elsewhere, zero included).
// The adjoint is linear in P, so one kernel shape serves both directions: never a scatter, no float atomics anywhere.
//
// A workgroup of 256 threads walks tiles of LGN_TR consecutive rows.  W_k (row stride C + 1 words; the backward loads it
// transposed, so that both directions read it along consecutive lanes) and b_k stay in LDS for the launch.  Gather: one
// wave a row; the wave is cut into 64 / lpr sub-groups of lpr lanes (lpr: the power of two that holds C / 4), a lane
// holds four columns, sub-group s sums the entries s, s + 64 / lpr, ... in two alternating chains, and the sub-groups'
// sums meet in a fixed butterfly.  The dense layer of a tile runs over all 256 threads from the tile's rows in LDS.
// Skewed rows: a row longer than LGN_CHUNK entries is not gathered by its tile.  A launch of its own gives every chunk of
// LGN_CHUNK entries to one wave, which stores the chunk's sum; the row's owner adds those sums in chunk order.  The value
// of a row is then a function of its entries, C and LGN_CHUNK alone -- not of the grid, nor of which rows share a tile.
// The caller names the long rows (ascending) with their chunk offsets: the graph is fixed, the plan is made once.
// A row that is long but not named is summed whole by its owner: correct, slower.
// Entries whose column lies outside 0 .. N - 1 are skipped, ids outside their table score 0: nothing is read out of bounds.
// dW_k | db_k: every thread keeps its elements of the sum over ALL tiles of its workgroup in registers and stores them
// once, into the workgroup's row of the partial buffer; the caller reduces the rows in ascending order.  The 256 threads
// are cut into 256 / dp groups of dp lanes (dp: the power of two from 32 up that holds C); a lane owns one column d of
// dW_k, its group a run of ceil(C / groups) rows c -- at most 16 accumulators up to C = 64, 64 beyond (two builds).
#include "common.h"

#define LGN_CHUNK 128       // entries one wave sums; a longer row is split
#define LGN_MAXC 128        // widest row
#define LGN_TR 16           // rows of a tile: 4 waves, 4 rows each
#define LGN_MAX_PARTS 2048  // workgroups of the backward launch = rows of the partial buffer
#define LGN_MAX_GRID 2048   // workgroups of the forward launch
#define LGN_SLOPE 0.2f

static bool lgn_c_ok(int C) { return C >= 4 && C <= LGN_MAXC && C % 4 == 0; }
static int lgn_lpr_log2(int C) {
  int l = 0;
  while ((1 << l) < C / 4) ++l;
  return l;
}
static long lgn_lds_floats(int C, int backward) { return (long)C * (C + 1) + C + (long)LGN_TR * C * (backward ? 3 : 1); }

extern "C" int clsr_lgn_row_chunk(void) { return LGN_CHUNK; }
extern "C" int clsr_lgn_max_width(void) { return LGN_MAXC; }
extern "C" int clsr_lgn_tile_rows(void) { return LGN_TR; }
extern "C" int clsr_lgn_supported(long N, long entries, int C) {
  return lgn_c_ok(C) && N > 0 && N < (1L << 31) && entries >= 0 && entries < (1L << 31);
}
extern "C" long clsr_lgn_lds_floats(int C, int backward) { return lgn_c_ok(C) ? lgn_lds_floats(C, backward) : 0; }
extern "C" int clsr_lgn_parts(long N) {
  if (N <= 0) return 0;
  const long tiles = (N + LGN_TR - 1) / LGN_TR;
  return (int)(tiles < LGN_MAX_PARTS ? tiles : LGN_MAX_PARTS);
}
extern "C" long clsr_lgn_part_floats(int C) { return lgn_c_ok(C) ? (long)C * C + C : 0; }
// the chunk sums of the long rows: [chunks][width]
extern "C" long clsr_lgn_workspace_floats(long chunks, int width) { return chunks > 0 && width > 0 ? chunks * width : 0; }

struct LgnCsr {
  const int* indptr; const int* indices; const float* values;     // values NULL: every entry 1
  const int* long_rows; const int* long_off; int nlong;           // rows longer than LGN_CHUNK, their chunk offsets
  float* long_part;                                               // [long_off[nlong]][width]
  long N; long ncols; long nchunks;
};

struct LgnArgs {
  LgnCsr g;
  const float* X;          // gathered rows [ncols][ldx]
  int ldx, C, lpr_log2;
  const float* W; const float* b;
  float* S_out; float* E_out; const float* E0; float* F_out;                      // forward
  const float* dF; const float* S; const float* Egate; float* dOut; float* part;  // backward
  float* out; int ldo;                                                            // plain product
};

// sum of values[e] X[indices[e]][4 qd .. 4 qd + 3] over e0 <= e < e1, in every lane of the wave that holds column quad qd
__device__ __forceinline__ f32x4 lgn_gather(const LgnCsr& g, long e0, long e1, const float* __restrict__ X, int ldx, int qd,
                                            int sub, int nsub, bool active, int lpr) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 a0 = zero, a1 = zero;
  if (active) {
    long e = e0 + sub;
    for (; e + nsub < e1; e += 2 * nsub) {
      const long j0 = g.indices[e], j1 = g.indices[e + nsub];
      const float v0 = g.values ? g.values[e] : 1.f, v1 = g.values ? g.values[e + nsub] : 1.f;
      const bool k0 = j0 >= 0 && j0 < g.ncols, k1 = j1 >= 0 && j1 < g.ncols;
      const f32x4 x0 = k0 ? ld4(X + j0 * ldx + 4 * qd) : zero, x1 = k1 ? ld4(X + j1 * ldx + 4 * qd) : zero;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (k0) a0[q] = fmaf(v0, x0[q], a0[q]);
        if (k1) a1[q] = fmaf(v1, x1[q], a1[q]);
      }
    }
    if (e < e1) {
      const long j0 = g.indices[e];
      const float v0 = g.values ? g.values[e] : 1.f;
      if (j0 >= 0 && j0 < g.ncols) {
        const f32x4 x0 = ld4(X + j0 * ldx + 4 * qd);
#pragma unroll
        for (int q = 0; q < 4; ++q) a0[q] = fmaf(v0, x0[q], a0[q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v = a0[q] + a1[q];
    for (int o = lpr; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    a0[q] = v;
  }
  return a0;
}

// the whole sum of row r (all lanes of the wave call it together): gathered, or the chunk sums of a named long row
__device__ __forceinline__ f32x4 lgn_row(const LgnCsr& g, long r, const float* __restrict__ X, int ldx, int width, int qd,
                                         int sub, int nsub, bool active, int lpr) {
  const long e0 = g.indptr[r], e1 = g.indptr[r + 1];
  if (e1 - e0 > LGN_CHUNK && g.nlong > 0) {
    int lo = 0, hi = g.nlong - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (g.long_rows[mid] < r) lo = mid + 1; else hi = mid;
    }
    if (g.long_rows[lo] == r) {
      long c0 = g.long_off[lo], c1 = g.long_off[lo + 1];
      if (c0 < 0) c0 = 0;
      if (c1 > g.nchunks) c1 = g.nchunks;     // (a plan that names more chunks than the workspace holds)
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      if (active)
#pragma unroll 8
        for (long c = c0; c < c1; ++c) {      // (independent loads, the adds in chunk order)
          const f32x4 p = ld4(g.long_part + c * width + 4 * qd);
#pragma unroll
          for (int q = 0; q < 4; ++q) s[q] += p[q];
        }
      return s;
    }
  }
  return lgn_gather(g, e0, e1, X, ldx, qd, sub, nsub, active, lpr);
}

// one wave a chunk of a long row: long_part[chunk] = the chunk's sum
__global__ void __launch_bounds__(256) lgn_long_kernel(LgnArgs a, int width) {
  const LgnCsr& g = a.g;
  const int lane = threadIdx.x & 63, lpr = 1 << a.lpr_log2, nsub = 64 >> a.lpr_log2;
  const int qd = lane & (lpr - 1), sub = lane >> a.lpr_log2;
  const bool active = 4 * qd < width;
  const long task = (long)blockIdx.x * 4 + (threadIdx.x >> 6), ntask = g.long_off[g.nlong];
  if (task >= ntask || task >= g.nchunks) return;
  int lo = 0, hi = g.nlong - 1;        // the last row whose first chunk is at or before the task
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g.long_off[mid] <= task) lo = mid; else hi = mid - 1;
  }
  const long r = g.long_rows[lo];
  long e0 = 0, e1 = 0;
  if (r >= 0 && r < g.N) {
    e0 = g.indptr[r] + (task - g.long_off[lo]) * LGN_CHUNK;
    e1 = g.indptr[r + 1];
    if (e1 > e0 + LGN_CHUNK) e1 = e0 + LGN_CHUNK;
  }
  const f32x4 s = lgn_gather(g, e0, e1, a.X, a.ldx, qd, sub, nsub, active, lpr);
  if (sub == 0 && active) st4(g.long_part + task * width + 4 * qd, s);
}

// out[r][0 .. width) = the sum of row r: the product alone (the category gradient: segments of item rows, values NULL)
__global__ void __launch_bounds__(256) lgn_rows_kernel(LgnArgs a, int width) {
  const LgnCsr& g = a.g;
  const int lane = threadIdx.x & 63, lpr = 1 << a.lpr_log2, nsub = 64 >> a.lpr_log2;
  const int qd = lane & (lpr - 1), sub = lane >> a.lpr_log2;
  const bool active = 4 * qd < width;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < g.N; r += (long)gridDim.x * 4) {
    const f32x4 s = lgn_row(g, r, a.X, a.ldx, width, qd, sub, nsub, active, lpr);
    if (sub == 0 && active) st4(a.out + r * a.ldo + 4 * qd, s);
  }
}

template <bool BWD, int NA>
__global__ void __launch_bounds__(256) lgn_layer_kernel(LgnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LgnCsr& g = a.g;
  const int C = a.C, C1 = C + 1, C4 = C >> 2, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lpr = 1 << a.lpr_log2, nsub = 64 >> a.lpr_log2, qd = lane & (lpr - 1), sub = lane >> a.lpr_log2;
  const bool active = qd < C4;
  float* Wl = lds;                     // forward [c][d] = W[c][d]; backward [d][k] = W[k][d]; row stride C + 1
  float* bl = Wl + C * C1;
  float* Tt = bl + C;                  // the tile's gathered sums [LGN_TR][C]
  float* St = Tt + LGN_TR * C;         // backward: the tile's own rows of S_k and P_k
  float* Pt = St + LGN_TR * C;
  for (int e = tid; e < C * C; e += 256) {
    const int r = e / C, c = e - r * C;
    if (BWD) Wl[c * C1 + r] = a.W[e]; else Wl[r * C1 + c] = a.W[e];
  }
  if (!BWD) for (int e = tid; e < C; e += 256) bl[e] = a.b[e];
  // backward: this thread's column of d W_k and its run of rows (NA: the most a run can hold)
  const int dpl = C <= 32 ? 5 : C <= 64 ? 6 : 7, dd = tid & ((1 << dpl) - 1), rg = tid >> dpl, ngr = 256 >> dpl;
  const int cpg = (C + ngr - 1) / ngr, c0 = rg * cpg;
  float acc[NA], accb = 0.f;
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = 0.f;
  const long ntiles = (g.N + LGN_TR - 1) / LGN_TR;
  const float third = 1.0f / 3.0f;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long r0 = t * LGN_TR;
    const int nt = (int)(g.N - r0 < LGN_TR ? g.N - r0 : LGN_TR);
    __syncthreads();       // the weights are in place; the previous tile's readers are done
    for (int i = wave; i < nt; i += 4) {
      const f32x4 s = lgn_row(g, r0 + i, a.X, C, C, qd, sub, nsub, active, lpr);
      if (sub == 0 && active) {
        st4(Tt + i * C + 4 * qd, s);
        if (!BWD && a.S_out) st4(a.S_out + (r0 + i) * C + 4 * qd, s);
      }
    }
    if (BWD)
      for (int e = tid; e < nt * C4; e += 256) {
        const int i = e / C4, c = (e - i * C4) * 4;
        st4(St + i * C + c, ld4(a.S + (r0 + i) * C + c));
        st4(Pt + i * C + c, ld4(a.X + (r0 + i) * C + c));
      }
    __syncthreads();
    // ---- the dense layer over the tile: four chains over the input columns (C is a multiple of 4)
    for (int e = tid; e < nt * C; e += 256) {
      const int i = e / C, d = e - i * C;
      const float* x = Tt + i * C;
      const float* w = Wl + d;
      float a0 = BWD ? 0.f : bl[d], a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int c = 0; c < C; c += 4) {
        a0 = fmaf(x[c], w[c * C1], a0);
        a1 = fmaf(x[c + 1], w[(c + 1) * C1], a1);
        a2 = fmaf(x[c + 2], w[(c + 2) * C1], a2);
        a3 = fmaf(x[c + 3], w[(c + 3) * C1], a3);
      }
      const float z = (a0 + a1) + (a2 + a3);
      const long o = (r0 + i) * C + d;
      if (!BWD) {
        const float y = z > 0.f ? z : LGN_SLOPE * z;
        a.E_out[o] = y;
        if (a.F_out) a.F_out[o] = ((a.E0[o] + a.X[o]) + y) * third;
      } else {
        float v = fmaf(a.dF[o], third, z);
        if (a.Egate) v *= a.Egate[o] > 0.f ? 1.f : LGN_SLOPE;
        a.dOut[o] = v;
      }
    }
    if (BWD) {
      // ---- d W_k [c][d] += sum over the tile's rows of S[r][c] P[r][d]; d b_k [d] += sum of P[r][d]
      if (dd < C)
        for (int r = 0; r < nt; ++r) {
          const float p = Pt[r * C + dd];
          const float* sr = St + r * C + c0;
          accb += p;
#pragma unroll
          for (int i = 0; i < NA; ++i)
            if (i < cpg && c0 + i < C) acc[i] = fmaf(sr[i], p, acc[i]);
        }
    }
  }
  if (BWD) {
    float* part = a.part + (long)blockIdx.x * (C * C + C);
    if (dd < C) {
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (i < cpg && c0 + i < C) part[(c0 + i) * C + dd] = acc[i];
      if (rg == 0) part[C * C + dd] = accb;
    }
  }
}

// out = scale * d * lrelu'(E): P of the last layer from dF (scale 1 / 3)
__global__ void lgn_gate_kernel(const float* __restrict__ d, const float* __restrict__ E, long n4, float scale,
                                float* __restrict__ out) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long)gridDim.x * 256) {
    const f32x4 v = ld4(d + 4 * e), y = ld4(E + 4 * e);
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = scale * v[q] * (y[q] > 0.f ? 1.f : LGN_SLOPE);
    st4(out + 4 * e, o);
  }
}

// 16 lanes a line: logit = F[u] . F[Vu + i]; with dlogit also the un-merged rows d F[u] = dlogit F[Vu + i], d F[Vu + i] = dlogit F[u]
template <bool BWD>
__global__ void __launch_bounds__(256) lgn_score_kernel(const int* __restrict__ users, int udiv, const int* __restrict__ items,
                                                        const float* __restrict__ F, long Vu, long Vi, int C, long B,
                                                        float* __restrict__ logit, const float* __restrict__ dlogit,
                                                        float* __restrict__ d_user, float* __restrict__ d_item,
                                                        int* __restrict__ uid_out) {
  const int q = threadIdx.x & 15;
  for (long l = (long)blockIdx.x * 16 + (threadIdx.x >> 4); l < (B + 15) / 16 * 16; l += (long)gridDim.x * 16) {
    const bool in = l < B;
    const long u = in ? users[l / udiv] : 0, i = in ? items[l] : 0;
    const bool ok = in && u >= 0 && u < Vu && i >= 0 && i < Vi;
    const float* fu = F + u * C;
    const float* fi = F + (Vu + i) * C;
    if (!BWD) {
      float acc = 0.f;
      if (ok)
        for (int c = 4 * q; c < C; c += 64) {
          const f32x4 x = ld4(fu + c), y = ld4(fi + c);
          acc = fmaf(x[0], y[0], acc); acc = fmaf(x[1], y[1], acc); acc = fmaf(x[2], y[2], acc); acc = fmaf(x[3], y[3], acc);
        }
      acc = row16_sum(acc);
      if (in && q == 0) logit[l] = acc;
    } else if (in) {
      const float d = dlogit[l];
      for (int c = 4 * q; c < C; c += 64) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 x = ok ? ld4(fu + c) : z, y = ok ? ld4(fi + c) : z;
        st4(d_user + l * C + c, y * d);
        st4(d_item + l * C + c, x * d);
      }
      if (q == 0) uid_out[l] = (int)u;
    }
  }
}

static void lgn_fill_csr(LgnCsr& g, const int* indptr, const int* indices, const float* values, const int* long_rows,
                        const int* long_off, int nlong, long nchunks, float* workspace, long N, long ncols) {
  g.indptr = indptr; g.indices = indices; g.values = values; g.long_rows = long_rows; g.long_off = long_off;
  g.nlong = nlong; g.long_part = workspace; g.N = N; g.ncols = ncols; g.nchunks = nchunks;
}

#define LGN_CHECK_CSR()                                                                                         \
  CLSR_CHECK_ARG(indptr && indices && N > 0 && N < (1L << 31));                                                 \
  CLSR_CHECK_ARG(nlong >= 0 && nchunks >= 0 && nchunks < (1L << 31) && (nlong == 0) == (nchunks == 0));         \
  CLSR_CHECK_ARG(nlong == 0 || (long_rows && long_off && workspace && ((uintptr_t)workspace & 15) == 0))

static int lgn_launch_long(const LgnArgs& a, long nchunks, int width, hipStream_t s) {
  if (a.g.nlong == 0) return CLSR_OK;
  hipLaunchKernelGGL(lgn_long_kernel, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, s, a, width);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

template <bool BWD, int NA>
static int lgn_launch_layer(const LgnArgs& a, unsigned grid, hipStream_t s) {
  const size_t bytes = (size_t)lgn_lds_floats(a.C, BWD) * sizeof(float);
  if (bytes > 65536) {    // past 64 KB of dynamic LDS the kernel has to be told, once per device (the widest rows only)
    static bool raised[64] = {};
    int dev = 0;
    CLSR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !raised[dev]) {
      CLSR_HIP(hipFuncSetAttribute((const void*)lgn_layer_kernel<BWD, NA>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(lgn_lds_floats(LGN_MAXC, BWD) * sizeof(float))));
      if (dev >= 0 && dev < 64) raised[dev] = true;
    }
  }
  hipLaunchKernelGGL((lgn_layer_kernel<BWD, NA>), dim3(grid), dim3(256), bytes, s, a);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_lgn_layer_fwd(const int* indptr, const int* indices, const float* values, const int* long_rows,
                                  const int* long_off, int nlong, long nchunks, long N, int C, const float* E_in,
                                  const float* W, const float* b, float* S_out, float* E_out, const float* E0,
                                  float* F_out, float* workspace, void* stream) {
  CLSR_CHECK_ARG(lgn_c_ok(C));
  LGN_CHECK_CSR();
  CLSR_CHECK_ARG(values && E_in && W && b && E_out && (!F_out || E0));
  CLSR_CHECK_ARG((((uintptr_t)E_in | (uintptr_t)S_out | (uintptr_t)E_out) & 15) == 0 && E_out != E_in && S_out != E_in);
  LgnArgs a = {};
  lgn_fill_csr(a.g, indptr, indices, values, long_rows, long_off, nlong, nchunks, workspace, N, N);
  a.X = E_in; a.ldx = C; a.C = C; a.lpr_log2 = lgn_lpr_log2(C); a.W = W; a.b = b;
  a.S_out = S_out; a.E_out = E_out; a.E0 = E0; a.F_out = F_out;
  hipStream_t s = (hipStream_t)stream;
  int rc = lgn_launch_long(a, nchunks, C, s);
  if (rc) return rc;
  const long tiles = (N + LGN_TR - 1) / LGN_TR;
  return lgn_launch_layer<false, 1>(a, (unsigned)(tiles < LGN_MAX_GRID ? tiles : LGN_MAX_GRID), s);
}

extern "C" int clsr_lgn_layer_bwd(const int* indptr, const int* indices, const float* values, const int* long_rows,
                                  const int* long_off, int nlong, long nchunks, long N, int C, const float* P,
                                  const float* W, const float* dF, const float* S, const float* E_gate, float* d_out,
                                  float* partial, float* workspace, void* stream) {
  CLSR_CHECK_ARG(lgn_c_ok(C));
  LGN_CHECK_CSR();
  CLSR_CHECK_ARG(values && P && W && dF && S && d_out && partial && d_out != P);
  CLSR_CHECK_ARG((((uintptr_t)P | (uintptr_t)S) & 15) == 0);
  LgnArgs a = {};
  lgn_fill_csr(a.g, indptr, indices, values, long_rows, long_off, nlong, nchunks, workspace, N, N);
  a.X = P; a.ldx = C; a.C = C; a.lpr_log2 = lgn_lpr_log2(C); a.W = W;
  a.dF = dF; a.S = S; a.Egate = E_gate; a.dOut = d_out; a.part = partial;
  hipStream_t s = (hipStream_t)stream;
  int rc = lgn_launch_long(a, nchunks, C, s);
  if (rc) return rc;
  if (C <= 64) return lgn_launch_layer<true, 16>(a, (unsigned)clsr_lgn_parts(N), s);
  return lgn_launch_layer<true, 64>(a, (unsigned)clsr_lgn_parts(N), s);
}

extern "C" int clsr_lgn_rows_sum(const int* indptr, const int* indices, const float* values, const int* long_rows,
                                 const int* long_off, int nlong, long nchunks, long N, long ncols, const float* X, int ldx,
                                 int width, float* out, int ldo, float* workspace, void* stream) {
  CLSR_CHECK_ARG(lgn_c_ok(width) && ldx >= width && ldo >= width && ldx % 4 == 0 && ldo % 4 == 0);
  LGN_CHECK_CSR();
  CLSR_CHECK_ARG(X && out && ncols > 0 && ncols < (1L << 31) && (((uintptr_t)X | (uintptr_t)out) & 15) == 0);
  LgnArgs a = {};
  lgn_fill_csr(a.g, indptr, indices, values, long_rows, long_off, nlong, nchunks, workspace, N, ncols);
  a.X = X; a.ldx = ldx; a.C = width; a.lpr_log2 = lgn_lpr_log2(width); a.out = out; a.ldo = ldo;
  hipStream_t s = (hipStream_t)stream;
  int rc = lgn_launch_long(a, nchunks, width, s);
  if (rc) return rc;
  const long blocks = (N + 3) / 4;
  hipLaunchKernelGGL(lgn_rows_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, a, width);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_lgn_gate(const float* d, const float* E, long n, float scale, float* out, void* stream) {
  CLSR_CHECK_ARG(d && E && out && n > 0 && n % 4 == 0 && (((uintptr_t)d | (uintptr_t)E | (uintptr_t)out) & 15) == 0);
  const long blocks = (n / 4 + 255) / 256;
  hipLaunchKernelGGL(lgn_gate_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, d,
                     E, n / 4, scale, out);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

#define LGN_CHECK_SCORE()                                                                                    \
  CLSR_CHECK_ARG(lgn_c_ok(C) && users && items && F && ((uintptr_t)F & 15) == 0 && user_div >= 1);            \
  CLSR_CHECK_ARG(B > 0 && B < (1L << 31) && Vu > 0 && Vi > 0 && Vu + Vi < (1L << 31));                        \
  const long blocks_ = (B + 15) / 16

extern "C" int clsr_lgn_score(const int* users, int user_div, const int* items, const float* F, long Vu, long Vi, int C,
                              long B, float* logit, void* stream) {
  LGN_CHECK_SCORE();
  CLSR_CHECK_ARG(logit);
  hipLaunchKernelGGL(lgn_score_kernel<false>, dim3((unsigned)(blocks_ < 4096 ? blocks_ : 4096)), dim3(256), 0,
                     (hipStream_t)stream, users, user_div, items, F, Vu, Vi, C, B, logit, nullptr, nullptr, nullptr, nullptr);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_lgn_logit_bwd(const int* users, int user_div, const int* items, const float* F, long Vu, long Vi, int C,
                                  long B, const float* dlogit, float* d_user, float* d_item, int* user_ids, void* stream) {
  LGN_CHECK_SCORE();
  CLSR_CHECK_ARG(dlogit && d_user && d_item && user_ids && (((uintptr_t)d_user | (uintptr_t)d_item) & 15) == 0);
  hipLaunchKernelGGL(lgn_score_kernel<true>, dim3((unsigned)(blocks_ < 4096 ? blocks_ : 4096)), dim3(256), 0,
                     (hipStream_t)stream, users, user_div, items, F, Vu, Vi, C, B, nullptr, dlogit, d_user, d_item, user_ids);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---- the two per-step statistics of the model on top of the propagation; per-workgroup doubles, added up in ascending
// workgroup order by one thread: no atomics, two runs give the same bits
#define LGN_STAT_BLOCKS 256

// the involved-row regulariser over any table of rows (F's item part: through the graph; the raw cate_embedding): for every
// flagged row, dF += l2 F; part = sum F^2
__global__ void __launch_bounds__(256) lgn_reg_kernel(const unsigned char* __restrict__ flags, const float* __restrict__ F,
                                                      float* __restrict__ dF, long V, int C, float l2,
                                                      double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  double acc = 0.0;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < V; r += (long)gridDim.x * 4) {
    if (!flags[r]) continue;
    for (int c = 4 * lane; c < C; c += 256) {
      const f32x4 f = ld4(F + r * C + c);
      f32x4 g = ld4(dF + r * C + c);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        g[q] = fmaf(l2, f[q], g[q]);
        acc += (double)f[q] * f[q];
      }
      st4(dF + r * C + c, g);
    }
  }
  const double v = block256_sum_d(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// squared norms of dE0's three pieces: user rows | item rows, columns 0 .. Di | item rows, columns Di .. C
__global__ void __launch_bounds__(256) lgn_sumsq_kernel(const float* __restrict__ X, long Vu, long N, int C, int Di,
                                                        double* __restrict__ part) {
  __shared__ double red[3][4];
  const int C4 = C >> 2;
  double acc[3] = {0.0, 0.0, 0.0};
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < N * C4; e += (long)gridDim.x * 256) {
    const long r = e / C4;
    const int c = (int)(e - r * C4) * 4;
    const f32x4 x = ld4(X + r * C + c);
    const double s = ((double)x[0] * x[0] + (double)x[1] * x[1]) + ((double)x[2] * x[2] + (double)x[3] * x[3]);
    if (r < Vu) acc[0] += s; else if (c < Di) acc[1] += s; else acc[2] += s;
  }
  const double v0 = block256_sum_d(acc[0], red[0]), v1 = block256_sum_d(acc[1], red[1]), v2 = block256_sum_d(acc[2], red[2]);
  if (threadIdx.x == 0) {
    part[3 * blockIdx.x] = v0; part[3 * blockIdx.x + 1] = v1; part[3 * blockIdx.x + 2] = v2;
  }
}

// out_q = sum over the workgroups of part[b * nq + q]
__global__ void lgn_stats_finish_kernel(const double* __restrict__ part, int nb, int nq, double* o0, double* o1, double* o2) {
  const int q = threadIdx.x;
  if (q >= nq) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += part[(long)b * nq + q];
  double* o = q == 0 ? o0 : q == 1 ? o1 : o2;
  o[0] = s;
}

// reg_loss += l2 / 2 * sum; sumsq (the squared norm of the added gradient rows l2 F) = l2^2 * sum
__global__ void lgn_reg_finish_kernel(const double* __restrict__ part, int nb, double l2, double* reg_loss, double* sumsq) {
  if (threadIdx.x) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += part[b];
  reg_loss[0] += 0.5 * l2 * s;
  if (sumsq) sumsq[0] = l2 * l2 * s;
}

extern "C" long clsr_lgn_stats_workspace_doubles(void) { return 3 * LGN_STAT_BLOCKS; }

extern "C" int clsr_lgn_reg_rows(const unsigned char* flags, const float* F, float* dF, long V, int C, float l2,
                                 double* workspace, double* reg_loss, double* sumsq, void* stream) {
  CLSR_CHECK_ARG(lgn_c_ok(C) && flags && F && dF && workspace && reg_loss && V > 0 && V < (1L << 31));
  CLSR_CHECK_ARG((((uintptr_t)F | (uintptr_t)dF) & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
  const long blocks = (V + 3) / 4;
  const int nb = (int)(blocks < LGN_STAT_BLOCKS ? blocks : LGN_STAT_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lgn_reg_kernel, dim3(nb), dim3(256), 0, s, flags, F, dF, V, C, l2, workspace);
  CLSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(lgn_reg_finish_kernel, dim3(1), dim3(64), 0, s, workspace, nb, (double)l2, reg_loss, sumsq);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

extern "C" int clsr_lgn_grad_sumsq(const float* dE0, long Vu, long N, int C, int Di, double* workspace, double* ss_user,
                                   double* ss_item, double* ss_cate, void* stream) {
  CLSR_CHECK_ARG(lgn_c_ok(C) && dE0 && workspace && ss_user && ss_item && ss_cate && ((uintptr_t)dE0 & 15) == 0);
  CLSR_CHECK_ARG(Vu > 0 && N > Vu && N < (1L << 31) && Di > 0 && Di < C && Di % 4 == 0 && ((uintptr_t)workspace & 7) == 0);
  const long blocks = (N * (C / 4) + 255) / 256;
  const int nb = (int)(blocks < LGN_STAT_BLOCKS ? blocks : LGN_STAT_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lgn_sumsq_kernel, dim3(nb), dim3(256), 0, s, dE0, Vu, N, C, Di, workspace);
  CLSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(lgn_stats_finish_kernel, dim3(1), dim3(64), 0, s, workspace, nb, 3, ss_user, ss_item, ss_cate);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}
