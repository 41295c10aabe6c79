// Feature-distance term of the self-supervised pretraining stage (train.py:480-483, trainer.train_step):
// d = torch.dist(encoder_features, imnet_features, p=2) = ||a - b||_2 over two fp32 NHWC tensors of one shape, and its gradient
// da = g * (a - b) / d (0 where d == 0, torch's norm backward).  HBM-bound: one pass over both operands with 16-byte loads.
// The reduction is deterministic and free of atomics: every block sums a fixed set of elements in double, a one-block launch
// combines the block partials in a fixed order and takes the square root on the device (nothing syncs with the host).
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)

constexpr int FD_MAX_BLOCKS = 1024;

// blocks of the partial-sum launch for `units` loads: ~8 per thread, at most FD_MAX_BLOCKS; a function of the size alone, so the
// summation order (and the result's bits) does not depend on anything else
inline int fd_blocks(long units) {
  const long nb = (units + 256L * 8 - 1) / (256L * 8);
  return (int)(nb < 1 ? 1 : (nb > FD_MAX_BLOCKS ? FD_MAX_BLOCKS : nb));
}
inline bool fd_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The operands as `rows` rows of `cols` floats with pitches lda / ldb (a dense pair is one row of M*C floats).  vec: the first
// 4 * (cols / 4) floats of a row are read as float4, the rest of the row (its tail) as floats.
__global__ __launch_bounds__(256) void feat_dist_partial_kernel(const float* a, long lda, const float* b, long ldb, long rows,
                                                                long cols, int vec, double* part) {
  SEGSDE_SMEM;
  double* sh = reinterpret_cast<double*>(segsde_smem);
  const long q = vec ? cols / 4 : 0, tail = cols - 4 * q;
  const long stride = (long)gridDim.x * 256;
  double acc = 0.0;
  const long nv = rows * q;
  for (long u = blockIdx.x * 256L + threadIdx.x; u < nv; u += stride) {
    const long m = rows == 1 ? 0 : u / q, j = u - m * q;
    const float4 x = *reinterpret_cast<const float4*>(a + m * lda + 4 * j);
    const float4 y = *reinterpret_cast<const float4*>(b + m * ldb + 4 * j);
    const double d0 = (double)x.x - (double)y.x, d1 = (double)x.y - (double)y.y;
    const double d2 = (double)x.z - (double)y.z, d3 = (double)x.w - (double)y.w;
    acc += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const long nt = rows * tail;
  for (long u = blockIdx.x * 256L + threadIdx.x; u < nt; u += stride) {
    const long m = rows == 1 ? 0 : u / tail, c = 4 * q + (u - m * tail);
    const double d = (double)a[m * lda + c] - (double)b[m * ldb + c];
    acc += d * d;
  }
  const double r = segsde_block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// 256 lanes sum strided subsets of the partials, then a fixed-order tree; out = sqrt(total)
__global__ __launch_bounds__(256) void feat_dist_finalize_kernel(const double* part, int n, float* out) {
  SEGSDE_SMEM;
  double* sh = reinterpret_cast<double*>(segsde_smem);
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += 256) s += part[i];
  sh[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) out[0] = (float)sqrt(sh[0]);
}

// da = (a - b) * s with s = g / d, 0 where d == 0 -- the order of torch's norm backward (self * (grad / norm).masked_fill_(norm == 0, 0))
__global__ __launch_bounds__(256) void feat_dist_backward_kernel(const float* a, long lda, const float* b, long ldb, long rows,
                                                                 long cols, int vec, const float* dist, const float* grad,
                                                                 float* da, long ldda) {
  const float dn = dist[0];
  const float s = dn == 0.f ? 0.f : grad[0] / dn;
  const long q = vec ? cols / 4 : 0, tail = cols - 4 * q;
  const long stride = (long)gridDim.x * 256;
  const long nv = rows * q;
  for (long u = blockIdx.x * 256L + threadIdx.x; u < nv; u += stride) {
    const long m = rows == 1 ? 0 : u / q, j = u - m * q;
    const float4 x = *reinterpret_cast<const float4*>(a + m * lda + 4 * j);
    const float4 y = *reinterpret_cast<const float4*>(b + m * ldb + 4 * j);
    *reinterpret_cast<float4*>(da + m * ldda + 4 * j) =
        make_float4((x.x - y.x) * s, (x.y - y.y) * s, (x.z - y.z) * s, (x.w - y.w) * s);
  }
  const long nt = rows * tail;
  for (long u = blockIdx.x * 256L + threadIdx.x; u < nt; u += stride) {
    const long m = rows == 1 ? 0 : u / tail, c = 4 * q + (u - m * tail);
    da[m * ldda + c] = (a[m * lda + c] - b[m * ldb + c]) * s;
  }
}

struct FdShape { long rows, cols, lda, ldb, ldd; int vec; long units; };

// dense operands (every pitch == C) are one row of M*C floats; float4 loads need 16-byte aligned bases and, with more than one
// row, pitches that keep every row aligned
FdShape fd_shape(const float* a, int lda, const float* b, int ldb, const float* d, int ldd, long M, int C) {
  FdShape s;
  const bool dense = lda == C && ldb == C && (!d || ldd == C);
  s.rows = dense ? 1 : M;
  s.cols = dense ? M * (long)C : C;
  s.lda = lda; s.ldb = ldb; s.ldd = ldd;
  const bool aligned = fd_al16(a) && fd_al16(b) && (!d || fd_al16(d));
  const bool pitches = dense || (lda % 4 == 0 && ldb % 4 == 0 && (!d || ldd % 4 == 0));
  s.vec = aligned && pitches && s.cols >= 4;
  s.units = s.vec ? s.rows * (s.cols / 4 + s.cols % 4) : s.rows * s.cols;
  return s;
}

}  // namespace

extern "C" size_t segsde_feat_dist_workspace(long M, int C) {
  return (size_t)fd_blocks(M * (long)(C > 0 ? C : 1)) * sizeof(double);
}

extern "C" int segsde_feat_dist_forward(const float* a, int lda, const float* b, int ldb, long M, int C, float* out, void* ws,
                                        size_t ws_bytes, void* stream) {
  if (!a || !b || !out || !ws) return SEGSDE_ERR_NULL;
  if (M <= 0 || C <= 0 || lda < C || ldb < C) return SEGSDE_ERR_SHAPE;
  if (ws_bytes < segsde_feat_dist_workspace(M, C)) return SEGSDE_ERR_WORKSPACE;
  const FdShape s = fd_shape(a, lda, b, ldb, nullptr, C, M, C);
  const int nb = fd_blocks(s.units);
  hipLaunchKernelGGL(feat_dist_partial_kernel, dim3(nb), dim3(256), 4 * sizeof(double), ST(stream), a, s.lda, b, s.ldb, s.rows,
                     s.cols, s.vec, (double*)ws);
  SEGSDE_CHECK_LAUNCH();
  hipLaunchKernelGGL(feat_dist_finalize_kernel, dim3(1), dim3(256), 256 * sizeof(double), ST(stream), (const double*)ws, nb, out);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_feat_dist_backward(const float* a, int lda, const float* b, int ldb, long M, int C, const float* dist,
                                         const float* grad, float* da, int ldda, void* stream) {
  if (!a || !b || !dist || !grad || !da) return SEGSDE_ERR_NULL;
  if (M <= 0 || C <= 0 || lda < C || ldb < C || ldda < C) return SEGSDE_ERR_SHAPE;
  const FdShape s = fd_shape(a, lda, b, ldb, da, ldda, M, C);
  long nb = (s.units + 1023) / 1024;
  nb = nb < 1 ? 1 : (nb > 8192 ? 8192 : nb);
  hipLaunchKernelGGL(feat_dist_backward_kernel, dim3((int)nb), dim3(256), 0, ST(stream), a, s.lda, b, s.ldb, s.rows, s.cols, s.vec,
                     dist, grad, da, s.ldd);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}
