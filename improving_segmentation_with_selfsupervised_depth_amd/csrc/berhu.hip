// BerHu pseudo-depth distillation loss (loss.py:5-15 of the reference; the only depth loss of the run that trains the label-selection
// model, experiments.py:229-301, and a term of every DepthMix validation, train.py:870-878):
//   a = |t - x| * m      (x, t replaced by log(1 + .) first when apply_log)
//   C = threshold * max(a) over the whole tensor
//   loss = mean over ALL elements of  a  where a <= C,  (a^2 + C^2) / (2 C)  otherwise
// The reference reads max(a) on the host (.item()); here nothing returns to the host.  Forward = three launches: block maxima of a
// into the workspace; every block folds those maxima itself (a few hundred floats from L2, the minmax_partial / minmax_apply pattern
// of depthmix.hip), forms C and sums its share of the loss in double; one block folds the block sums in a fixed order.  Backward =
// one launch that recomputes a from x, t, m and the saved C: no map is kept between the passes.  8 bytes per element and forward
// pass, 12 for the backward pass, 4 more per pass with a mask tensor.
// The own-car crop of both callers ("rows >= int(0.9 H) do not count") needs no mask tensor: element e of a [.., H, W] tensor is
// kept iff e % (H W) < keep_rows W, carried along the grid-stride loop by additions.
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)
constexpr int BH_THREADS = 256;
constexpr int BH_CUS = 256;                       // compute units of the MI355X, the one target of this library
constexpr int BH_MAX_BLOCKS = 3 * BH_CUS;         // 12 waves per CU; larger tensors take further trips of the grid-stride loop
constexpr int BH_ELEMS_PER_BLOCK = 4 * BH_THREADS;

struct bh_args {
  const float* x;
  const float* t;
  const float* m;                                 // or null
  long n;
  long HW, keepW;                                 // crop: H * W and keep_rows * W; HW = 0 without one
  int vec;                                        // every pointer of the launch is 16-byte aligned
};

inline int bh_blocks(long n) {
  const long nb = (n + BH_ELEMS_PER_BLOCK - 1) / BH_ELEMS_PER_BLOCK;
  return (int)(nb < 1 ? 1 : (nb > BH_MAX_BLOCKS ? BH_MAX_BLOCKS : nb));
}

template <bool LOG>
__device__ __forceinline__ float bh_diff(float x, float t) {
  if (LOG) { x = logf(1.f + x); t = logf(1.f + t); }
  return t - x;
}

// out[e] = f(x[e], t[e], m[e]) for every element this thread owns (STORE) or just f(...); m is 1 without a mask tensor and 0 inside
// the crop.  Quads of four elements as 16-byte accesses plus a scalar tail of n % 4 elements, or element by element.
template <bool STORE, class F>
__device__ __forceinline__ void bh_for_each(const bh_args& A, float* out, F&& f) {
  const long gtid = blockIdx.x * (long)BH_THREADS + threadIdx.x;
  const long nthr = (long)gridDim.x * BH_THREADS;
  const long HW = A.HW, keepW = A.keepW;
  if (A.vec) {
    const long n4 = A.n >> 2;
    long r = 0, rstep = 0;                        // r = (4 q) % HW, kept up by additions
    if (HW > 0) { r = (gtid * 4) % HW; rstep = (nthr * 4) % HW; }
    for (long q = gtid; q < n4; q += nthr) {
      const float4 x4 = reinterpret_cast<const float4*>(A.x)[q];
      const float4 t4 = reinterpret_cast<const float4*>(A.t)[q];
      float4 m4 = make_float4(1.f, 1.f, 1.f, 1.f);
      if (A.m) m4 = reinterpret_cast<const float4*>(A.m)[q];
      if (HW > 0) {
        long ri = r;
        if (ri >= keepW) m4.x = 0.f;
        ri = ri + 1 == HW ? 0 : ri + 1;
        if (ri >= keepW) m4.y = 0.f;
        ri = ri + 1 == HW ? 0 : ri + 1;
        if (ri >= keepW) m4.z = 0.f;
        ri = ri + 1 == HW ? 0 : ri + 1;
        if (ri >= keepW) m4.w = 0.f;
        r += rstep;
        if (r >= HW) r -= HW;
      }
      float4 o;
      o.x = f(x4.x, t4.x, m4.x); o.y = f(x4.y, t4.y, m4.y); o.z = f(x4.z, t4.z, m4.z); o.w = f(x4.w, t4.w, m4.w);
      if (STORE) reinterpret_cast<float4*>(out)[q] = o;
    }
    const long e = (n4 << 2) + gtid;              // the tail: the first n % 4 threads of the grid
    if (e < A.n) {
      float m = A.m ? A.m[e] : 1.f;
      if (HW > 0 && e % HW >= keepW) m = 0.f;
      const float o = f(A.x[e], A.t[e], m);
      if (STORE) out[e] = o;
    }
  } else {
    long r = 0, rstep = 0;
    if (HW > 0) { r = gtid % HW; rstep = nthr % HW; }
    for (long e = gtid; e < A.n; e += nthr) {
      float m = A.m ? A.m[e] : 1.f;
      if (HW > 0) {
        if (r >= keepW) m = 0.f;
        r += rstep;
        if (r >= HW) r -= HW;
      }
      const float o = f(A.x[e], A.t[e], m);
      if (STORE) out[e] = o;
    }
  }
}

// the maximum of the block's four wave maxima (sh: 4 floats of LDS), in every thread
__device__ __forceinline__ float bh_block_max(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// ------------------------------------------------------------------------------------------------------------------ 1. maxima
template <bool LOG>
__global__ __launch_bounds__(BH_THREADS) void berhu_max_kernel(bh_args A, float* pmax /*[gridDim.x]*/) {
  SEGSDE_SMEM;
  float mx = -INFINITY;                           // a block (a thread) without an element leaves the fold untouched
  bh_for_each<false>(A, nullptr, [&](float x, float t, float m) {
    mx = fmaxf(mx, fabsf(bh_diff<LOG>(x, t)) * m);
    return 0.f;
  });
  mx = bh_block_max(mx, reinterpret_cast<float*>(segsde_smem));
  if (threadIdx.x == 0) pmax[blockIdx.x] = mx;
}

// ------------------------------------------------------------------------------------------------------------------ 2. sums
// C as the reference forms it: threshold * max in double (Python floats), rounded to fp32 where it meets the fp32 tensor -- in the
// comparison, as C * C (rounded from the double product) and as 2 C.
template <bool LOG>
__global__ __launch_bounds__(BH_THREADS) void berhu_sum_kernel(bh_args A, const float* pmax, int nblk, double threshold,
                                                               double* psum /*[gridDim.x]*/, float* state /*{max, C}*/) {
#pragma clang fp contract(off)
  SEGSDE_SMEM;
  float* shf = reinterpret_cast<float*>(segsde_smem);
  double* shd = reinterpret_cast<double*>(segsde_smem + 32);
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < nblk; i += BH_THREADS) mx = fmaxf(mx, pmax[i]);
  mx = bh_block_max(mx, shf);
  const double Cd = threshold * (double)mx;
  const float C = (float)Cd, CC = (float)(Cd * Cd), C2 = (float)(2.0 * Cd);
  if (blockIdx.x == 0 && threadIdx.x == 0) { state[0] = mx; state[1] = C; }
  double acc = 0.0;
  bh_for_each<false>(A, nullptr, [&](float x, float t, float m) {
    const float a = fabsf(bh_diff<LOG>(x, t)) * m;
    acc += (double)(a <= C ? a : (a * a + CC) / C2);
    return 0.f;
  });
  const double r = segsde_block_sum(acc, shd);
  if (threadIdx.x == 0) psum[blockIdx.x] = r;
}

// ------------------------------------------------------------------------------------------------------------------ 3. fold
// thread i adds the sums of blocks i, i + 256, ... in ascending order, then the butterfly of segsde_block_sum: one order in every run
__global__ __launch_bounds__(BH_THREADS) void berhu_finish_kernel(const double* psum, int nblk, long n, float* loss) {
  SEGSDE_SMEM;
  double a = 0.0;
  for (int i = threadIdx.x; i < nblk; i += BH_THREADS) a += psum[i];
  a = segsde_block_sum(a, reinterpret_cast<double*>(segsde_smem));
  if (threadIdx.x == 0) loss[0] = (float)(a / (double)n);
}

// ------------------------------------------------------------------------------------------------------------------ backward
// dx = g / n * -sign(t - x) * m * (a <= C ? 1 : a / C)  [/ (1 + x) with the logarithm]; C is a constant (the reference detaches it
// with .item()).  a == 0 (masked, cropped, t == x; everything when max(a) = 0) gives exactly 0.
template <bool LOG>
__global__ __launch_bounds__(BH_THREADS) void berhu_backward_kernel(bh_args A, const float* state, const float* gscale, float* dx) {
#pragma clang fp contract(off)
  const float C = state[1];
  const float gn = gscale[0] / (float)A.n;
  bh_for_each<true>(A, dx, [&](float x, float t, float m) {
    const float d = bh_diff<LOG>(x, t);
    const float a = fabsf(d) * m;
    if (a == 0.f) return 0.f;
    float v = gn * m;
    if (!(a <= C)) v = v * (a / C);
    v = d > 0.f ? -v : v;
    if (LOG) v = v / (1.f + x);
    return v;
  });
}

inline bool bh_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool bh_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// the checks both directions share
inline int bh_check(const float* x, const float* t, const float* m, long n, int H, int W, int keep_rows) {
  if (n <= 0 || keep_rows < -1) return SEGSDE_ERR_SHAPE;
  if (keep_rows >= 0) {
    if (H <= 0 || W <= 0 || keep_rows > H || n % ((long)H * W) != 0) return SEGSDE_ERR_SHAPE;
  }
  if (!bh_aligned4(x) || !bh_aligned4(t) || !bh_aligned4(m)) return SEGSDE_ERR_UNSUPPORTED;
  return 0;
}
inline bh_args bh_make_args(const float* x, const float* t, const float* m, long n, int H, int W, int keep_rows, const float* dx) {
  bh_args A;
  A.x = x; A.t = t; A.m = m; A.n = n;
  A.HW = keep_rows >= 0 ? (long)H * W : 0;
  A.keepW = keep_rows >= 0 ? (long)keep_rows * W : 0;
  A.vec = n >= 4 && bh_aligned16(x) && bh_aligned16(t) && bh_aligned16(m) && bh_aligned16(dx);
  return A;
}
}  // namespace

extern "C" size_t segsde_berhu_workspace(long n) {
  if (n <= 0) return 0;
  return (size_t)bh_blocks(n) * (sizeof(double) + sizeof(float));
}

extern "C" int segsde_berhu_forward(const float* input, const float* target, const float* mask, long n, int H, int W, int keep_rows,
                                    int apply_log, double threshold, float* loss, float* state, void* ws, size_t ws_bytes,
                                    void* stream) {
  if (!input || !target || !loss || !state || !ws) return SEGSDE_ERR_NULL;
  const int bad = bh_check(input, target, mask, n, H, W, keep_rows);
  if (bad == SEGSDE_ERR_SHAPE) return bad;
  if (!(threshold > 0.0 && threshold < INFINITY)) return SEGSDE_ERR_SHAPE;                   // negated: NaN is refused
  if (ws_bytes < segsde_berhu_workspace(n)) return SEGSDE_ERR_WORKSPACE;
  if (bad) return bad;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) || !bh_aligned4(loss) || !bh_aligned4(state)) return SEGSDE_ERR_UNSUPPORTED;
  const bh_args A = bh_make_args(input, target, mask, n, H, W, keep_rows, nullptr);
  const int nblk = bh_blocks(n);
  double* psum = static_cast<double*>(ws);
  float* pmax = reinterpret_cast<float*>(psum + nblk);
  if (apply_log) hipLaunchKernelGGL(berhu_max_kernel<true>, dim3(nblk), dim3(BH_THREADS), 64, ST(stream), A, pmax);
  else hipLaunchKernelGGL(berhu_max_kernel<false>, dim3(nblk), dim3(BH_THREADS), 64, ST(stream), A, pmax);
  SEGSDE_CHECK_LAUNCH();
  if (apply_log)
    hipLaunchKernelGGL(berhu_sum_kernel<true>, dim3(nblk), dim3(BH_THREADS), 64, ST(stream), A, (const float*)pmax, nblk, threshold,
                       psum, state);
  else
    hipLaunchKernelGGL(berhu_sum_kernel<false>, dim3(nblk), dim3(BH_THREADS), 64, ST(stream), A, (const float*)pmax, nblk, threshold,
                       psum, state);
  SEGSDE_CHECK_LAUNCH();
  hipLaunchKernelGGL(berhu_finish_kernel, dim3(1), dim3(BH_THREADS), 64, ST(stream), (const double*)psum, nblk, n, loss);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_berhu_backward(const float* input, const float* target, const float* mask, long n, int H, int W, int keep_rows,
                                     int apply_log, const float* state, const float* gscale, float* dinput, void* stream) {
  if (!input || !target || !state || !gscale || !dinput) return SEGSDE_ERR_NULL;
  const int bad = bh_check(input, target, mask, n, H, W, keep_rows);
  if (bad) return bad;
  if (!bh_aligned4(state) || !bh_aligned4(gscale) || !bh_aligned4(dinput)) return SEGSDE_ERR_UNSUPPORTED;
  const bh_args A = bh_make_args(input, target, mask, n, H, W, keep_rows, dinput);
  const int nblk = bh_blocks(n);
  if (apply_log) hipLaunchKernelGGL(berhu_backward_kernel<true>, dim3(nblk), dim3(BH_THREADS), 0, ST(stream), A, state, gscale, dinput);
  else hipLaunchKernelGGL(berhu_backward_kernel<false>, dim3(nblk), dim3(BH_THREADS), 0, ST(stream), A, state, gscale, dinput);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}
