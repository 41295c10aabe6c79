// Mix masks for a whole batch (Trainer.generate_mix_mask, train.py:573-584 "class" and 605-636 "depth" / "depthhist"): the reference
// walks the batch in Python, one image at a time; here every mode is a fixed number of launches whatever the batch size.
//
// "depthhist" (train.py:616-636) per image: x = log(1 + d); np.histogram(x, bins=100, density=True); max_depth = right edge of the
// highest bin below the top one whose density exceeds 1.5; min_depth = left edge of the first bin at which the cumulated density
// passes 0.4 of the total; threshold = u * (max_depth - min_depth) + min_depth; mask = d >= threshold.  np.histogram of float32 data
// is restated in fp32 arithmetic (see dh_edge): three launches -- block minima / maxima into the workspace; every block folds its
// image's partials, builds the 101 edges in LDS, bins its pixels (an arithmetic guess, corrected against the edge table, so that
// membership is edges[k] <= x < edges[k + 1] whatever the guess) into block-private LDS counters and flushes them with integer
// atomics; one block turns the counters into densities (double) and thresholds.  No float atomics: two calls give the same bits.
// "class" (ClassMix, train.py:573-584): the pixel count of every class id per image (the host draws the classes from the ids that
// are present: numpy's generator is the reference's random stream), then mask = selected[image][id].
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)
constexpr int MM_THREADS = 256;
constexpr int MM_PIX_PER_BLOCK = 16 * MM_THREADS;
constexpr int MM_MAX_PARTS = 256;                 // blocks per image at most: one partial per thread when they are folded
constexpr int MM_MAX_BLOCKS = 2048;               // 8 blocks per compute unit; larger batches take further trips of the pixel loops
constexpr int MM_BINS = 100;                      // np.histogram(..., bins=100), train.py:619
constexpr int MM_IDS = 256;                       // class ids -1 .. 254 in slots 0 .. 255
// Neighbouring pixels of a smooth depth map or of a segmentation fall into the same counter.  Lane l counts in copy l % 16 of the
// block's counters ([counter][copy], so that the 16 copies of one counter lie in 16 banks): at most four lanes of a wave meet on
// one address.
constexpr int MM_COPIES = 16;
constexpr int MM_FINISH_WAVES = 16;               // images the one block of the last "depthhist" launch takes per trip

inline int mm_parts(int B, long HW) {
  const long want = (HW + MM_PIX_PER_BLOCK - 1) / MM_PIX_PER_BLOCK;
  long cap = MM_MAX_BLOCKS / B;
  cap = cap < 1 ? 1 : (cap > MM_MAX_PARTS ? MM_MAX_PARTS : cap);
  return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}
inline bool mm_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// f(value) for every pixel of image blockIdx.y that this thread owns; quads as 16-byte loads when the image rows allow it
template <class F>
__device__ __forceinline__ void mm_for_each(const float* img, long HW, int vec, F&& f) {
  const long t = blockIdx.x * (long)MM_THREADS + threadIdx.x, nt = (long)gridDim.x * MM_THREADS;
  if (vec) {
    const long n4 = HW >> 2;
    for (long q = t; q < n4; q += nt) {
      const float4 v = reinterpret_cast<const float4*>(img)[q];
      f(v.x); f(v.y); f(v.z); f(v.w);
    }
  } else {
    for (long e = t; e < HW; e += nt) f(img[e]);
  }
}

// minimum and maximum over the block (sh: 8 floats of LDS), in every thread
__device__ __forceinline__ void mm_block_minmax(float& mn, float& mx, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = mn; sh[4 + (threadIdx.x >> 6)] = mx; }
  __syncthreads();
  mn = fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
  mx = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
}

// np.histogram's range and edges for float32 data (numpy 2.2): a constant image widens its range by 0.5 on both sides;
// edges = np.linspace(lo, hi, 101) in float32 = float32(k) * ((hi - lo) / 100) + lo, product and sum rounded separately, the last
// edge set to hi itself.
__device__ __forceinline__ void dh_range(float& lo, float& hi, float& step) {
#pragma clang fp contract(off)
  if (lo == hi) { lo = lo - 0.5f; hi = hi + 0.5f; }
  step = (hi - lo) / (float)MM_BINS;
}
__device__ __forceinline__ float dh_edge(int k, float lo, float hi, float step) {
#pragma clang fp contract(off)
  if (k >= MM_BINS) return hi;
  const float prod = (float)k * step;
  return prod + lo;
}

// ------------------------------------------------------------------------------------------------------ depthhist 1: block min / max
template <bool LOG>
__global__ __launch_bounds__(MM_THREADS) void dh_minmax_kernel(const float* d, long HW, int vec, float* pmm /*[B][P][2]*/,
                                                               unsigned* counts /*[B][100]: zeroed here*/) {
  SEGSDE_SMEM;
  const int b = blockIdx.y;
  float mn = INFINITY, mx = -INFINITY;            // a thread without a pixel leaves the fold untouched
  mm_for_each(d + (long)b * HW, HW, vec, [&](float v) {
    if (LOG) v = logf(1.0f + v);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  });
  mm_block_minmax(mn, mx, reinterpret_cast<float*>(segsde_smem));
  if (threadIdx.x == 0) {
    float* o = pmm + ((long)b * gridDim.x + blockIdx.x) * 2;
    o[0] = mn; o[1] = mx;
  }
  if (blockIdx.x == 0 && threadIdx.x < MM_BINS) counts[(long)b * MM_BINS + threadIdx.x] = 0u;
}

// ------------------------------------------------------------------------------------------------------ depthhist 2: the histogram
template <bool LOG>
__global__ __launch_bounds__(MM_THREADS) void dh_hist_kernel(const float* d, long HW, int vec, const float* pmm, float* lohi /*[B][2]*/,
                                                             unsigned* counts) {
#pragma clang fp contract(off)
  SEGSDE_SMEM;
  float* red = reinterpret_cast<float*>(segsde_smem);                     // 8 floats
  float* edges = red + 8;                                                 // 101 (104) floats
  unsigned* h = reinterpret_cast<unsigned*>(edges + 104);                 // [100][16]
  const int b = blockIdx.y, P = gridDim.x;
  float lo = INFINITY, hi = -INFINITY, step;
  for (int i = threadIdx.x; i < P; i += MM_THREADS) {
    lo = fminf(lo, pmm[((long)b * P + i) * 2]);
    hi = fmaxf(hi, pmm[((long)b * P + i) * 2 + 1]);
  }
  mm_block_minmax(lo, hi, red);
  dh_range(lo, hi, step);
  if (threadIdx.x <= MM_BINS) edges[threadIdx.x] = dh_edge(threadIdx.x, lo, hi, step);
  for (int i = threadIdx.x; i < MM_BINS * MM_COPIES; i += MM_THREADS) h[i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) { lohi[2 * b] = lo; lohi[2 * b + 1] = hi; }
  __syncthreads();
  const float scale = (float)MM_BINS / (hi - lo);
  const int copy = threadIdx.x & (MM_COPIES - 1);
  int run_k = 0;                                  // consecutive pixels of a thread that share a bin are counted with one atomic
  unsigned run_n = 0;
  mm_for_each(d + (long)b * HW, HW, vec, [&](float v) {
    if (LOG) v = logf(1.0f + v);
    // the guess only has to be a bin index; the two loops settle membership on the edges (edges[k] <= v < edges[k + 1], the last
    // bin closed on the right); NaN ends in bin 0
    const float g = fminf(fmaxf((v - lo) * scale, 0.f), (float)(MM_BINS - 1));
    int k = (int)g;
    while (k > 0 && v < edges[k]) --k;
    while (k < MM_BINS - 1 && v >= edges[k + 1]) ++k;
    if (k != run_k) {
      if (run_n) atomicAdd(&h[run_k * MM_COPIES + copy], run_n);
      run_k = k;
      run_n = 0;
    }
    ++run_n;
  });
  if (run_n) atomicAdd(&h[run_k * MM_COPIES + copy], run_n);
  __syncthreads();
  if (threadIdx.x < MM_BINS) {
    unsigned s = 0;
#pragma unroll
    for (int c = 0; c < MM_COPIES; ++c) s += h[threadIdx.x * MM_COPIES + ((c + threadIdx.x) & (MM_COPIES - 1))];
    if (s) atomicAdd(&counts[(long)b * MM_BINS + threadIdx.x], s);
  }
}

// ------------------------------------------------------------------------------------------------------ depthhist 3: thresholds
// One block of 16 waves.  Wave w takes images w, w + 16, ...: density of bin k = n_k / double(edges[k + 1] - edges[k]) / N (the edge difference in
// fp32 first, as np.diff of the float32 edges), the running sum in ascending k like np.cumsum, both scans.  Then one thread walks
// the images in order: an image without a qualifying bin takes the max_depth of the image before it, the first image its own top
// edge (the reference reuses the stale value silently and dies on the first image), and threshold = u * (max - min) + min in fp32.
__global__ __launch_bounds__(64 * MM_FINISH_WAVES) void dh_finish_kernel(const unsigned* counts, const float* lohi, const float* u, int B, long HW,
                                                               float* table /*[B][4]*/) {
#pragma clang fp contract(off)
  SEGSDE_SMEM;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* cum = reinterpret_cast<double*>(segsde_smem) + w * 128;
  for (int b0 = 0; b0 < B; b0 += MM_FINISH_WAVES) {
    const int b = b0 + w;
    const bool on = b < B;
    float lo = 0.f, hi = 1.f;
    if (on) { lo = lohi[2 * b]; hi = lohi[2 * b + 1]; }
    const float step = (hi - lo) / (float)MM_BINS;
    const int k0 = lane, k1 = lane + 64;
    const bool two = k1 < MM_BINS;
    double h0 = 0.0, h1 = 0.0;
    if (on) {
      const float w0 = dh_edge(k0 + 1, lo, hi, step) - dh_edge(k0, lo, hi, step);
      h0 = (double)counts[(long)b * MM_BINS + k0] / (double)w0 / (double)HW;
      if (two) {
        const float w1 = dh_edge(k1 + 1, lo, hi, step) - dh_edge(k1, lo, hi, step);
        h1 = (double)counts[(long)b * MM_BINS + k1] / (double)w1 / (double)HW;
      }
    }
    cum[k0] = h0;
    if (two) cum[k1] = h1;
    __syncthreads();
    if (lane == 0) {
      double c = 0.0;
      for (int k = 0; k < MM_BINS; ++k) { c += cum[k]; cum[k] = c; }
    }
    __syncthreads();
    const double sum = cum[MM_BINS - 1];
    int top = -1, first = MM_BINS;
    if (h0 > 1.5) top = k0;                                               // k0 <= 63
    if (two && k1 <= MM_BINS - 2 && h1 > 1.5) top = k1;                   // the top bin is excluded (train.py:620-621)
    if (two && cum[k1] / sum > 0.4) first = k1;
    if (cum[k0] / sum > 0.4) first = k0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int t2 = __shfl_xor(top, o), f2 = __shfl_xor(first, o);
      top = t2 > top ? t2 : top;
      first = f2 < first ? f2 : first;
    }
    if (lane == 0 && on) {
      float* row = table + 4L * b;
      row[0] = dh_edge(first, lo, hi, step);
      row[1] = top >= 0 ? dh_edge(top + 1, lo, hi, step) : hi;
      row[3] = top >= 0 ? 1.f : 0.f;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float cur = 0.f;
    for (int b = 0; b < B; ++b) {
      float* row = table + 4L * b;
      if (b > 0 && row[3] == 0.f) row[1] = cur;
      cur = row[1];
      const float prod = u[b] * (cur - row[0]);
      row[2] = prod + row[0];
    }
  }
}

// ------------------------------------------------------------------------------------------------------ masks
__global__ __launch_bounds__(MM_THREADS) void thr_mask_batch_kernel(const float* d, long HW, int vec, const float* thr, long thr_stride,
                                                                    float* mask) {
  const int b = blockIdx.y;
  const float t = thr[b * thr_stride];
  const float* img = d + (long)b * HW;
  float* out = mask + (long)b * HW;
  const long tid = blockIdx.x * (long)MM_THREADS + threadIdx.x, nt = (long)gridDim.x * MM_THREADS;
  if (vec) {
    const long n4 = HW >> 2;
    for (long q = tid; q < n4; q += nt) {
      const float4 v = reinterpret_cast<const float4*>(img)[q];
      reinterpret_cast<float4*>(out)[q] = make_float4(v.x >= t ? 1.f : 0.f, v.y >= t ? 1.f : 0.f, v.z >= t ? 1.f : 0.f, v.w >= t ? 1.f : 0.f);
    }
  } else {
    for (long e = tid; e < HW; e += nt) out[e] = img[e] >= t ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(MM_THREADS) void class_presence_kernel(const int64_t* pred, long HW, unsigned* counts /*[B][256]*/) {
  SEGSDE_SMEM;
  unsigned* h = reinterpret_cast<unsigned*>(segsde_smem);                 // [256][16]
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < MM_IDS * MM_COPIES; i += MM_THREADS) h[i] = 0u;
  __syncthreads();
  const int64_t* img = pred + (long)b * HW;
  const int copy = threadIdx.x & (MM_COPIES - 1);
  for (long e = blockIdx.x * (long)MM_THREADS + threadIdx.x; e < HW; e += (long)gridDim.x * MM_THREADS) {
    const int64_t v = img[e];
    if (v >= -1 && v <= MM_IDS - 2) atomicAdd(&h[((int)v + 1) * MM_COPIES + copy], 1u);
  }
  __syncthreads();
  unsigned s = 0;
#pragma unroll
  for (int c = 0; c < MM_COPIES; ++c) s += h[threadIdx.x * MM_COPIES + ((c + threadIdx.x) & (MM_COPIES - 1))];
  if (s) atomicAdd(&counts[(long)b * MM_IDS + threadIdx.x], s);
}

__global__ __launch_bounds__(MM_THREADS) void class_mask_batch_kernel(const int64_t* pred, long HW, const unsigned char* selected,
                                                                      int64_t* mask) {
  SEGSDE_SMEM;
  unsigned char* sel = segsde_smem;                                       // this image's 256 flags
  const int b = blockIdx.y;
  sel[threadIdx.x] = selected[(long)b * MM_IDS + threadIdx.x];
  __syncthreads();
  const int64_t* img = pred + (long)b * HW;
  int64_t* out = mask + (long)b * HW;
  for (long e = blockIdx.x * (long)MM_THREADS + threadIdx.x; e < HW; e += (long)gridDim.x * MM_THREADS) {
    const int64_t v = img[e];
    out[e] = (v >= -1 && v <= MM_IDS - 2) ? (int64_t)sel[(int)v + 1] : 0;
  }
}

inline int mm_shape(int B, long HW) {
  if (B < 1 || HW < 1 || HW >= (1L << 31)) return SEGSDE_ERR_SHAPE;
  return 0;
}
constexpr int MM_MAX_BATCH = 65535;               // the images are the grid's y dimension
}  // namespace

extern "C" size_t segsde_depth_hist_workspace(int B, long HW) {
  if (mm_shape(B, HW) || B > MM_MAX_BATCH) return 0;
  // block partials {min, max}, the range {lo, hi} per image, the counters of a call that does not ask for them
  return (size_t)B * ((size_t)mm_parts(B, HW) * 2 * sizeof(float) + 2 * sizeof(float) + MM_BINS * sizeof(unsigned));
}

extern "C" int segsde_depth_hist_thresholds(const float* depth, int B, long HW, int apply_log, const float* u, float* table,
                                            unsigned* counts, void* ws, size_t ws_bytes, void* stream) {
  if (!depth || !u || !table || !ws) return SEGSDE_ERR_NULL;
  if (mm_shape(B, HW)) return SEGSDE_ERR_SHAPE;
  if (B > MM_MAX_BATCH) return SEGSDE_ERR_UNSUPPORTED;
  if (ws_bytes < segsde_depth_hist_workspace(B, HW)) return SEGSDE_ERR_WORKSPACE;
  if (!mm_aligned(depth, 4) || !mm_aligned(u, 4) || !mm_aligned(table, 4) || !mm_aligned(counts, 4) || !mm_aligned(ws, 4))
    return SEGSDE_ERR_UNSUPPORTED;
  const int P = mm_parts(B, HW);
  float* pmm = static_cast<float*>(ws);
  float* lohi = pmm + (size_t)B * P * 2;
  unsigned* cnt = counts ? counts : reinterpret_cast<unsigned*>(lohi + (size_t)B * 2);
  const int vec = (HW & 3) == 0 && mm_aligned(depth, 16);
  const dim3 grid(P, B), block(MM_THREADS);
  if (apply_log) hipLaunchKernelGGL(dh_minmax_kernel<true>, grid, block, 64, ST(stream), depth, HW, vec, pmm, cnt);
  else hipLaunchKernelGGL(dh_minmax_kernel<false>, grid, block, 64, ST(stream), depth, HW, vec, pmm, cnt);
  SEGSDE_CHECK_LAUNCH();
  const size_t lds = (8 + 104) * sizeof(float) + MM_BINS * MM_COPIES * sizeof(unsigned);
  if (apply_log) hipLaunchKernelGGL(dh_hist_kernel<true>, grid, block, lds, ST(stream), depth, HW, vec, (const float*)pmm, lohi, cnt);
  else hipLaunchKernelGGL(dh_hist_kernel<false>, grid, block, lds, ST(stream), depth, HW, vec, (const float*)pmm, lohi, cnt);
  SEGSDE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dh_finish_kernel, dim3(1), dim3(64 * MM_FINISH_WAVES), MM_FINISH_WAVES * 128 * sizeof(double), ST(stream), (const unsigned*)cnt, (const float*)lohi,
                     u, B, HW, table);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_depth_threshold_mask_batch(const float* depth, int B, long HW, const float* thr, long thr_stride, float* mask,
                                                 void* stream) {
  if (!depth || !thr || !mask) return SEGSDE_ERR_NULL;
  if (mm_shape(B, HW) || thr_stride < 0) return SEGSDE_ERR_SHAPE;
  if (B > MM_MAX_BATCH || !mm_aligned(depth, 4) || !mm_aligned(thr, 4) || !mm_aligned(mask, 4)) return SEGSDE_ERR_UNSUPPORTED;
  const int vec = (HW & 3) == 0 && mm_aligned(depth, 16) && mm_aligned(mask, 16);
  hipLaunchKernelGGL(thr_mask_batch_kernel, dim3(mm_parts(B, HW), B), dim3(MM_THREADS), 0, ST(stream), depth, HW, vec, thr, thr_stride,
                     mask);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_class_presence(const int64_t* pred, int B, long HW, unsigned* counts, void* stream) {
  if (!pred || !counts) return SEGSDE_ERR_NULL;
  if (mm_shape(B, HW)) return SEGSDE_ERR_SHAPE;
  if (B > MM_MAX_BATCH || !mm_aligned(pred, 8) || !mm_aligned(counts, 4)) return SEGSDE_ERR_UNSUPPORTED;
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * MM_IDS * sizeof(unsigned), ST(stream));
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(class_presence_kernel, dim3(mm_parts(B, HW), B), dim3(MM_THREADS), MM_IDS * MM_COPIES * sizeof(unsigned), ST(stream),
                     pred, HW, counts);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_class_mask_batch(const int64_t* pred, int B, long HW, const unsigned char* selected, int64_t* mask, void* stream) {
  if (!pred || !selected || !mask) return SEGSDE_ERR_NULL;
  if (mm_shape(B, HW)) return SEGSDE_ERR_SHAPE;
  if (B > MM_MAX_BATCH || !mm_aligned(pred, 8) || !mm_aligned(mask, 8)) return SEGSDE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(class_mask_batch_kernel, dim3(mm_parts(B, HW), B), dim3(MM_THREADS), MM_IDS, ST(stream), pred, HW, selected, mask);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}
