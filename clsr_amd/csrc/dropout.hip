// Dropout of _fcn_net's hidden layers (gfx950): base_model.py _active_layer applies tf.nn.dropout in FRONT of the
// activation when user_dropout is set -- a = relu(dropout(bn(z))), keep = 1 - dropout[layer].
//
// The mask is a pure function of (seed, draw, layer, global row, column) (csrc/philox.h): it is never stored, the
// backward kernel draws it again.  seed and draw live in a 4-word device buffer `state` = {seed low, seed high, draw,
// 0}: the step bumps `draw` with one launch of its own, so that a replayed launch plan or a replayed hipGraph -- whose
// scalars are frozen -- still sees a new mask per step.  (Not the Adam clock: its tick may run early on a side stream.)
//
// No kernel here asks for LDS (small LDS-requesting launches queue behind the LDS-owning kernels of the step, see the
// note in csrc/p2p.hip) and none uses atomics: the batch-norm sums leave as one partial row per (workgroup, row slot),
// every thread adds its own rows in ascending order, so two runs are bit-identical.
#include "common.h"
#include "philox.h"

#define DROP_MAX_PARTS 512

__global__ void dropout_tick_kernel(unsigned int* __restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) state[2] = state[2] + 1u;
}

extern "C" int clsr_dropout_tick(unsigned int* state, void* stream) {
  CLSR_CHECK_ARG(state);
  hipLaunchKernelGGL(dropout_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// a[r, 4q..4q+3] = keep ? relu(scale * z + shift) * inv_keep : 0; one thread per 16-byte chunk, one Philox call each
__global__ void __launch_bounds__(256) bn_relu_dropout_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
    const unsigned int* __restrict__ state, unsigned int layer, unsigned int row0, unsigned int thr, float inv_keep,
    int total, int QC, float* __restrict__ a) {
  const unsigned int s0 = state[0], s1 = state[1], draw = state[2];
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int r = e / QC, q = e - r * QC;
    const clsr_u32x4 w = clsr_dropout_words(s0, s1, draw, layer, row0 + (unsigned int)r, (unsigned int)q);
    const f32x4 y = ld4(z + (long)e * 4) * ld4(scale + 4 * q) + ld4(shift + 4 * q);
    f32x4 o;
    o.x = (clsr_dropout_keep(w.x, thr) && y.x > 0.f) ? y.x * inv_keep : 0.f;
    o.y = (clsr_dropout_keep(w.y, thr) && y.y > 0.f) ? y.y * inv_keep : 0.f;
    o.z = (clsr_dropout_keep(w.z, thr) && y.z > 0.f) ? y.z * inv_keep : 0.f;
    o.w = (clsr_dropout_keep(w.w, thr) && y.w > 0.f) ? y.w * inv_keep : 0.f;
    st4(a + (long)e * 4, o);
  }
}

extern "C" int clsr_bn_relu_dropout_fwd(const float* z, const float* scale, const float* shift,
                                        const unsigned int* state, int layer, long row0, int thr, float inv_keep,
                                        long B, int C, float* a, void* stream) {
  CLSR_CHECK_ARG(z && scale && shift && state && a && B > 0 && layer >= 0 && row0 >= 0);
  CLSR_CHECK_ARG(thr >= 0 && thr <= (1 << 24) && inv_keep > 0.f);
  CLSR_CHECK_SUPPORTED(C % 4 == 0 && C >= 4 && C <= 1024 && B * (C / 4) < (1L << 31) - (1L << 24));
  const int QC = C / 4, total = (int)(B * QC);
  int blocks = clsr_cdiv(total, 256);
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(bn_relu_dropout_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, z, scale, shift,
                     state, (unsigned int)layer, (unsigned int)row0, (unsigned int)thr, inv_keep, total, QC, a);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// dy = da * mask * inv_keep * [scale * z + shift > 0]  (dy may alias da);
// bn_partial[p][0][c] = sum dy, bn_partial[p][1][c] = sum dy * xhat, xhat = (z - mean) * invstd -- the layout of
// clsr_mlp_out_bwd, with one part p = blockIdx.x * rpb + ty per (workgroup, row slot): thread (ty, q) owns the float4
// column q of rows p, p + parts, p + 2 parts, ... and writes its own eight sums.
__global__ void __launch_bounds__(256) bn_relu_dropout_bwd_kernel(
    const float* da, const float* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ mean, const float* __restrict__ invstd, const unsigned int* __restrict__ state,
    unsigned int layer, unsigned int row0, unsigned int thr, float inv_keep, int B, int C, float* dy,
    double* __restrict__ bn_partial) {
  const int QC = C >> 2, rpb = 256 / QC;
  const int ty = threadIdx.x / QC, q = threadIdx.x - ty * QC;
  if (ty >= rpb) return;
  const int parts = gridDim.x * rpb, p = blockIdx.x * rpb + ty;
  const unsigned int s0 = state[0], s1_ = state[1], draw = state[2];
  const f32x4 sc = ld4(scale + 4 * q), sh = ld4(shift + 4 * q), mu = ld4(mean + 4 * q), is = ld4(invstd + 4 * q);
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  for (int r = p; r < B; r += parts) {
    const long off = (long)r * C + 4 * q;
    const clsr_u32x4 w = clsr_dropout_words(s0, s1_, draw, layer, row0 + (unsigned int)r, (unsigned int)q);
    const f32x4 zz = ld4(z + off), g = ld4(da + off);
    const f32x4 y = zz * sc + sh;
    f32x4 d;
    d.x = (clsr_dropout_keep(w.x, thr) && y.x > 0.f) ? g.x * inv_keep : 0.f;
    d.y = (clsr_dropout_keep(w.y, thr) && y.y > 0.f) ? g.y * inv_keep : 0.f;
    d.z = (clsr_dropout_keep(w.z, thr) && y.z > 0.f) ? g.z * inv_keep : 0.f;
    d.w = (clsr_dropout_keep(w.w, thr) && y.w > 0.f) ? g.w * inv_keep : 0.f;
    st4(dy + off, d);
    const f32x4 xh = (zz - mu) * is;
    s1[0] += d.x; s1[1] += d.y; s1[2] += d.z; s1[3] += d.w;
    s2[0] += (double)d.x * xh.x; s2[1] += (double)d.y * xh.y;
    s2[2] += (double)d.z * xh.z; s2[3] += (double)d.w * xh.w;
  }
  double* o1 = bn_partial + ((long)p * 2 + 0) * C + 4 * q;
  double* o2 = bn_partial + ((long)p * 2 + 1) * C + 4 * q;
#pragma unroll
  for (int k = 0; k < 4; ++k) { o1[k] = s1[k]; o2[k] = s2[k]; }
}

static int drop_bwd_blocks(long B, int C) {
  const int rpb = 256 / (C / 4);
  long b = (B + rpb * 4 - 1) / (rpb * 4);
  const long cap = DROP_MAX_PARTS / rpb > 0 ? DROP_MAX_PARTS / rpb : 1;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

extern "C" int clsr_bn_relu_dropout_bwd_parts(long B, int C) {
  if (C % 4 || C < 4 || C > 1024 || B <= 0) return 0;
  return drop_bwd_blocks(B, C) * (256 / (C / 4));
}

extern "C" int clsr_bn_relu_dropout_bwd(const float* da, const float* z, const float* scale, const float* shift,
                                        const float* mean, const float* invstd, const unsigned int* state, int layer,
                                        long row0, int thr, float inv_keep, long B, int C, float* dy,
                                        double* bn_partial, void* stream) {
  CLSR_CHECK_ARG(da && z && scale && shift && mean && invstd && state && dy && bn_partial && B > 0 && layer >= 0 &&
                 row0 >= 0);
  CLSR_CHECK_ARG(thr >= 0 && thr <= (1 << 24) && inv_keep > 0.f);
  CLSR_CHECK_SUPPORTED(C % 4 == 0 && C >= 4 && C <= 1024 && B < (1L << 31) - 512);
  hipLaunchKernelGGL(bn_relu_dropout_bwd_kernel, dim3(drop_bwd_blocks(B, C)), dim3(256), 0, (hipStream_t)stream, da,
                     z, scale, shift, mean, invstd, state, (unsigned int)layer, (unsigned int)row0, (unsigned int)thr,
                     inv_keep, (int)B, C, dy, bn_partial);
  CLSR_CHECK_LAUNCH();
  return CLSR_OK;
}

// ---- the same generator on the host (no GPU needed): known-answer and mask tests
extern "C" int clsr_philox4x32_10_host(const unsigned int* ctr, const unsigned int* key, unsigned int* out) {
  CLSR_CHECK_ARG(ctr && key && out);
  const clsr_u32x4 o = clsr_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  out[0] = o.x; out[1] = o.y; out[2] = o.z; out[3] = o.w;
  return CLSR_OK;
}

// mask[r * C + c] = 1 (kept) / 0 of rows row0 ... row0 + B - 1 (HOST pointer, any C >= 1)
extern "C" int clsr_dropout_mask_host(unsigned long seed, unsigned int draw, int layer, long row0, long B, int C,
                                      int thr, unsigned char* mask) {
  CLSR_CHECK_ARG(mask && B > 0 && C > 0 && layer >= 0 && row0 >= 0 && thr >= 0 && thr <= (1 << 24));
  const uint32_t s0 = (uint32_t)(seed & 0xffffffffu), s1 = (uint32_t)(seed >> 32);
  for (long r = 0; r < B; ++r)
    for (int q = 0; 4 * q < C; ++q) {
      const clsr_u32x4 w = clsr_dropout_words(s0, s1, draw, (uint32_t)layer, (uint32_t)(row0 + r), (uint32_t)q);
      const uint32_t v[4] = {w.x, w.y, w.z, w.w};
      for (int k = 0; k < 4 && 4 * q + k < C; ++k)
        mask[r * C + 4 * q + k] = clsr_dropout_keep(v[k], (uint32_t)thr) ? 1 : 0;
    }
  return CLSR_OK;
}
