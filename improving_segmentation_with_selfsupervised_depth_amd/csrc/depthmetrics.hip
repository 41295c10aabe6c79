// Depth evaluation (the metrics MonodepthLoss.depth_metric_names lists): per image a validity mask, an optional crop, the
// prediction scaled by median(gt) / median(pred), a clamp, the seven errors.  The medians are EXACT order statistics: the float
// bits are mapped to an unsigned key of the same order and a most-significant-digit radix select (4 digits of 8 bits) narrows the
// key prefixes of the two middle ranks on the device -- per digit one counting pass (LDS histograms per block, folded into one
// per-image histogram by integer atomics, which commute) and one tiny launch that picks the digit.  No launch, grid size or copy
// depends on the data; every float sum is block partials folded in a fixed order.  Five passes over gt and pred: 40 bytes a pixel.
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)

constexpr int DM_THREADS = 256;
constexpr int DM_PIX_PER_BLOCK = 8192;          // 8 quads of 4 pixels per thread before another block is worth its histogram flush
constexpr int DM_MAX_BLOCKS = 1024;             // per image; larger images take further trips of the grid-stride loop
constexpr int DM_PASSES = 4, DM_BINS = 256;
constexpr int DM_NSUM = 7;                      // sum |d|/g, sum d^2/g, sum d^2, sum dlog^2, n_a1, n_a2, n_a3
constexpr int DM_STATE_WORDS = 16;              // per image: [tensor][rank]{prefix, remaining rank} = 8 words, n, padding
constexpr int DM_HIST_WORDS = DM_PASSES * 4 * DM_BINS;      // per image: [pass][tensor][rank][bin]

// what a block needs to know about the pixels it walks over: image b of gt / pred, the crop, and whether the crop is a run of
// whole rows whose first element has the same 16-byte phase in both tensors (then it is read as aligned float4)
struct dm_geom {
  int W, y0, x0, cw, vec;
  long HW, npix;                                // pixels of an image, pixels of the crop
  float min_depth, max_depth;
};

inline int dm_blocks(long npix) {
  const long nb = (npix + DM_PIX_PER_BLOCK - 1) / DM_PIX_PER_BLOCK;
  return (int)(nb < 1 ? 1 : (nb > DM_MAX_BLOCKS ? DM_MAX_BLOCKS : nb));
}

// IEEE order of the finite values as an unsigned order: negative numbers have all bits flipped, the others the sign bit set
__device__ __forceinline__ unsigned dm_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dm_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// f(g, p) for every VALID pixel of the crop of one image (gt, pred: the image's first element) that this thread owns
template <class F>
__device__ __forceinline__ void dm_for_each_valid(const float* gt, const float* pred, const dm_geom& G, F&& f) {
  const float lo = G.min_depth, hi = G.max_depth;
  const long stride = (long)gridDim.x * DM_THREADS;
  if (G.vec) {
    const float* g0 = gt + (long)G.y0 * G.W;
    const float* p0 = pred + (long)G.y0 * G.W;
    const long mis = (long)((reinterpret_cast<uintptr_t>(g0) >> 2) & 3);      // elements past a 16-byte boundary
    const long nq = (mis + G.npix + 3) / 4;
    for (long q = blockIdx.x * (long)DM_THREADS + threadIdx.x; q < nq; q += stride) {
      const long e0 = q * 4 - mis;                                            // < 0 only for the first quad
      if (e0 >= 0 && e0 + 4 <= G.npix) {
        const float4 g4 = *reinterpret_cast<const float4*>(g0 + e0);
        const float4 p4 = *reinterpret_cast<const float4*>(p0 + e0);
        if (g4.x > lo && g4.x < hi) f(g4.x, p4.x);
        if (g4.y > lo && g4.y < hi) f(g4.y, p4.y);
        if (g4.z > lo && g4.z < hi) f(g4.z, p4.z);
        if (g4.w > lo && g4.w < hi) f(g4.w, p4.w);
      } else {
        for (int i = 0; i < 4; ++i) {
          const long e = e0 + i;
          if (e < 0 || e >= G.npix) continue;
          const float g = g0[e];
          if (g > lo && g < hi) f(g, p0[e]);
        }
      }
    }
  } else {
    for (long e = blockIdx.x * (long)DM_THREADS + threadIdx.x; e < G.npix; e += stride) {
      const long off = (G.y0 + e / G.cw) * (long)G.W + G.x0 + e % G.cw;
      const float g = gt[off];
      if (g > lo && g < hi) f(g, pred[off]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ 1. count
// Digit `pass` (0 = the most significant 8 bits) of the keys whose higher digits equal the prefix of rank j of tensor t.  While
// the prefixes of the two ranks of a tensor agree (before the first digit: always) only histogram 0 is filled and both ranks
// read it.  grid (blocks, B); LDS: [tensor][rank][256] counts.
__global__ __launch_bounds__(DM_THREADS) void dm_count_kernel(const float* gt, const float* pred, dm_geom G, const unsigned* state,
                                                              unsigned* hist, int pass) {
  SEGSDE_SMEM;
  unsigned* h = reinterpret_cast<unsigned*>(segsde_smem);                     // [4][DM_BINS]
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < 4 * DM_BINS; i += DM_THREADS) h[i] = 0;
  const unsigned* st = state + (long)b * DM_STATE_WORDS;
  unsigned pg0 = 0, pg1 = 0, pp0 = 0, pp1 = 0;
  if (pass > 0) { pg0 = st[0]; pg1 = st[2]; pp0 = st[4]; pp1 = st[6]; }
  const int hs = 32 - 8 * pass, ds = 24 - 8 * pass;                           // prefix shift (32 at pass 0: not used), digit shift
  __syncthreads();
  if (pass == 0) {
    dm_for_each_valid(gt + b * G.HW, pred + b * G.HW, G, [&](float g, float p) {
      atomicAdd(h + (dm_key(g) >> 24), 1u);
      atomicAdd(h + 2 * DM_BINS + (dm_key(p) >> 24), 1u);
    });
  } else {
    dm_for_each_valid(gt + b * G.HW, pred + b * G.HW, G, [&](float g, float p) {
      const unsigned kg = dm_key(g), kp = dm_key(p);
      const unsigned hg = kg >> hs, hp = kp >> hs, dg = (kg >> ds) & 255u, dp = (kp >> ds) & 255u;
      if (hg == pg0) atomicAdd(h + dg, 1u);
      else if (hg == pg1) atomicAdd(h + DM_BINS + dg, 1u);
      if (hp == pp0) atomicAdd(h + 2 * DM_BINS + dp, 1u);
      else if (hp == pp1) atomicAdd(h + 3 * DM_BINS + dp, 1u);
    });
  }
  __syncthreads();
  unsigned* out = hist + ((long)b * DM_PASSES + pass) * 4 * DM_BINS;
  for (int i = threadIdx.x; i < 4 * DM_BINS; i += DM_THREADS)
    if (h[i]) atomicAdd(out + i, h[i]);
}

// ------------------------------------------------------------------------------------------------------------------ 2. narrow
// One block per image, wave w = (tensor, rank): the digit whose bin holds the rank.  Lane l owns bins 4l..4l+3; the lane sums go
// through LDS, every lane adds up the ones before it, and the one lane whose range holds the rank picks among its four bins.  An
// image without a valid pixel has no such lane: its state stays zero and the finish pass writes NaN.
__global__ __launch_bounds__(256) void dm_narrow_kernel(const unsigned* hist, unsigned* state, int pass) {
  SEGSDE_SMEM;
  unsigned* sums = reinterpret_cast<unsigned*>(segsde_smem);                  // [4][64]
  const int b = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63, t = w >> 1, j = w & 1;
  const unsigned* hb = hist + ((long)b * DM_PASSES + pass) * 4 * DM_BINS;
  unsigned* st = state + (long)b * DM_STATE_WORDS;
  unsigned prefix = 0, k = 0;
  const unsigned* h = hb + t * 2 * DM_BINS;
  if (pass > 0) {
    const unsigned p0 = st[t * 4], p1 = st[t * 4 + 2];
    prefix = j ? p1 : p0;
    k = st[t * 4 + j * 2 + 1];
    if (j == 1 && p0 != p1) h += DM_BINS;
  }
  unsigned c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = h[l * 4 + i];
  const unsigned own = c[0] + c[1] + c[2] + c[3];
  sums[w * 64 + l] = own;
  __syncthreads();                                                            // and: every state word is read before any is rewritten
  unsigned before = 0;
  for (int i = 0; i < 64; ++i) before += i < l ? sums[w * 64 + i] : 0u;
  if (pass == 0) {
    unsigned n = 0;
    for (int i = 0; i < 64; ++i) n += sums[i];                                // every valid pixel is in gt's first histogram
    k = n == 0 ? 0u : (j == 0 ? (n - 1) / 2 : n / 2);
    if (threadIdx.x == 0) st[8] = n;
  }
  if (k < before || k - before >= own) return;
  unsigned cum = before;                                                      // cum <= k throughout: no wrap
  int d = 0;
  if (k - cum >= c[0]) {
    cum += c[0]; d = 1;
    if (k - cum >= c[1]) {
      cum += c[1]; d = 2;
      if (k - cum >= c[2]) { cum += c[2]; d = 3; }
    }
  }
  st[t * 4 + j * 2] = (prefix << 8) | (unsigned)(l * 4 + d);
  st[t * 4 + j * 2 + 1] = k - cum;
}

// the medians and the ratio from the state after the last digit (every thread computes them: a dozen operations)
struct dm_scale { unsigned n; float med_gt, med_pred, ratio; };
__device__ __forceinline__ dm_scale dm_read_scale(const unsigned* st, int median_scaling, float scale) {
#pragma clang fp contract(off)
  dm_scale s;
  s.n = st[8];
  const float g_lo = dm_unkey(st[0]), g_hi = dm_unkey(st[2]), p_lo = dm_unkey(st[4]), p_hi = dm_unkey(st[6]);
  s.med_gt = (s.n & 1u) ? g_lo : (g_lo + g_hi) / 2.f;
  s.med_pred = (s.n & 1u) ? p_lo : (p_lo + p_hi) / 2.f;
  s.ratio = median_scaling ? scale * (s.med_gt / s.med_pred) : scale;
  return s;
}

// ------------------------------------------------------------------------------------------------------------------ 3. errors
// part: [B][gridDim.x][DM_NSUM] doubles
__global__ __launch_bounds__(DM_THREADS) void dm_error_kernel(const float* gt, const float* pred, dm_geom G, const unsigned* state,
                                                              int median_scaling, float scale, double* part) {
#pragma clang fp contract(off)
  SEGSDE_SMEM;
  double* red = reinterpret_cast<double*>(segsde_smem);
  const int b = blockIdx.y;
  const float ratio = dm_read_scale(state + (long)b * DM_STATE_WORDS, median_scaling, scale).ratio;
  const float lo = G.min_depth, hi = G.max_depth;
  double acc[DM_NSUM];
#pragma unroll
  for (int q = 0; q < DM_NSUM; ++q) acc[q] = 0.0;
  unsigned a1 = 0, a2 = 0, a3 = 0;                                            // a thread sees fewer than 2^32 / 256 pixels
  dm_for_each_valid(gt + b * G.HW, pred + b * G.HW, G, [&](float g, float pr) {
    const float p = fminf(fmaxf(pr * ratio, lo), hi);
    const float d = g - p, d2 = d * d;
    const float lg = logf(g) - logf(p);
    const float t = fmaxf(g / p, p / g);
    acc[0] += (double)(fabsf(d) / g);
    acc[1] += (double)(d2 / g);
    acc[2] += (double)d2;
    acc[3] += (double)(lg * lg);
    a1 += t < 1.25f;
    a2 += t < 1.5625f;
    a3 += t < 1.953125f;
  });
  acc[4] = (double)a1; acc[5] = (double)a2; acc[6] = (double)a3;
#pragma unroll
  for (int q = 0; q < DM_NSUM; ++q) {
    const double r = segsde_block_sum(acc[q], red);
    if (threadIdx.x == 0) part[((long)b * gridDim.x + blockIdx.x) * DM_NSUM + q] = r;
  }
}

// ------------------------------------------------------------------------------------------------------------------ 4. finish
// One block of DM_NSUM waves per image: wave q folds sum q.  Lane l adds the partials of blocks l, l + 64, ... in ascending order,
// then the 64 lane sums meet in the butterfly of segsde_wave_sum: the same order in every run.
__global__ __launch_bounds__(DM_NSUM * 64) void dm_finish_kernel(const double* part, int nblk, const unsigned* state,
                                                                 int median_scaling, float scale, double* table) {
  SEGSDE_SMEM;
  double* s = reinterpret_cast<double*>(segsde_smem);                         // [DM_NSUM]
  const int b = blockIdx.x, q = threadIdx.x >> 6, l = threadIdx.x & 63;
  double a = 0.0;
  for (int i = l; i < nblk; i += 64) a += part[((long)b * nblk + i) * DM_NSUM + q];
  a = segsde_wave_sum(a);
  if (l == 0) s[q] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const dm_scale sc = dm_read_scale(state + (long)b * DM_STATE_WORDS, median_scaling, scale);
  double* row = table + (long)b * SEGSDE_DEPTH_ERRORS_COLUMNS;
  if (sc.n == 0) {
    for (int c = 0; c < SEGSDE_DEPTH_ERRORS_COLUMNS; ++c) row[c] = (double)NAN;
    row[7] = 0.0;
    return;
  }
  const double n = (double)sc.n;
  row[0] = s[0] / n;
  row[1] = s[1] / n;
  row[2] = sqrt(s[2] / n);
  row[3] = sqrt(s[3] / n);
  row[4] = s[4] / n;
  row[5] = s[5] / n;
  row[6] = s[6] / n;
  row[7] = n;
  row[8] = s[4];
  row[9] = s[5];
  row[10] = s[6];
  row[11] = (double)sc.med_gt;
  row[12] = (double)sc.med_pred;
  row[13] = (double)sc.ratio;
}

inline long dm_crop_pixels(int y0, int y1, int x0, int x1) { return (long)(y1 - y0) * (x1 - x0); }
inline size_t dm_part_bytes(int B, int nblk) { return (size_t)B * nblk * DM_NSUM * sizeof(double); }
}  // namespace

// sized for the full image, so that one workspace serves every crop
extern "C" size_t segsde_depth_errors_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return dm_part_bytes(B, dm_blocks((long)H * W)) + (size_t)B * (DM_HIST_WORDS + DM_STATE_WORDS) * sizeof(unsigned);
}

extern "C" int segsde_depth_errors(const float* gt, const float* pred, int B, int H, int W, float min_depth, float max_depth,
                                   int median_scaling, float scale, int y0, int y1, int x0, int x1, double* table, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (!gt || !pred || !table || !ws) return SEGSDE_ERR_NULL;
  if (B <= 0 || H <= 0 || W <= 0) return SEGSDE_ERR_SHAPE;
  if (y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1) return SEGSDE_ERR_SHAPE;
  if (!(0.f <= min_depth && min_depth < max_depth)) return SEGSDE_ERR_SHAPE;                 // negated: NaN is refused
  if ((long)H * W >= (1L << 32) || B > 65535 || (reinterpret_cast<uintptr_t>(ws) & 7)) return SEGSDE_ERR_UNSUPPORTED;
  if (ws_bytes < segsde_depth_errors_workspace(B, H, W)) return SEGSDE_ERR_WORKSPACE;
  dm_geom G;
  G.W = W; G.y0 = y0; G.x0 = x0; G.cw = x1 - x0;
  G.HW = (long)H * W;
  G.npix = dm_crop_pixels(y0, y1, x0, x1);
  G.min_depth = min_depth; G.max_depth = max_depth;
  // whole rows, and the two tensors share their 16-byte phase (each image works out its own: an image pitch that is no multiple
  // of 4 elements moves it from image to image, in both tensors alike)
  G.vec = (G.cw == W) && (((reinterpret_cast<uintptr_t>(gt) ^ reinterpret_cast<uintptr_t>(pred)) & 15) == 0);
  const int nblk = dm_blocks(G.npix);                                        // <= the blocks the workspace was sized for
  double* part = static_cast<double*>(ws);
  unsigned* hist = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(ws) + dm_part_bytes(B, dm_blocks(G.HW)));
  unsigned* state = hist + (size_t)B * DM_HIST_WORDS;
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * (DM_HIST_WORDS + DM_STATE_WORDS) * sizeof(unsigned), ST(stream));
  if (e != hipSuccess) return (int)e;
  for (int pass = 0; pass < DM_PASSES; ++pass) {
    hipLaunchKernelGGL(dm_count_kernel, dim3(nblk, B), dim3(DM_THREADS), 4 * DM_BINS * sizeof(unsigned), ST(stream), gt, pred, G,
                       (const unsigned*)state, hist, pass);
    SEGSDE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dm_narrow_kernel, dim3(B), dim3(256), 4 * 64 * sizeof(unsigned), ST(stream), (const unsigned*)hist, state,
                       pass);
    SEGSDE_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(dm_error_kernel, dim3(nblk, B), dim3(DM_THREADS), 64, ST(stream), gt, pred, G, (const unsigned*)state,
                     median_scaling ? 1 : 0, scale, part);
  SEGSDE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dm_finish_kernel, dim3(B), dim3(DM_NSUM * 64), 64, ST(stream), (const double*)part, nblk, (const unsigned*)state,
                     median_scaling ? 1 : 0, scale, table);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}
