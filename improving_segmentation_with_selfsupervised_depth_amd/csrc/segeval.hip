// Validation of the segmentation head at LABEL resolution (train.py:836-851 with loss/loss.py:17-37 behind self.loss_fn) in one
// pass: for every label pixel the C logits are interpolated from the network's output grid (F.interpolate(..., mode="bilinear",
// align_corners=True): lerp_src of segsde_common.h, the arithmetic of resize_fwd_kernel bit for bit), then
//   argmax over the classes (strict >, the lowest index wins a tie: confusion_kernel's rule),
//   hist[C * label + argmax] += 1                      where 0 <= label < C,
//   loss sum += logsumexp(z) - z[label], count += 1    where label != ignore_index and 0 <= label < C,
//   ids[pixel] = argmax                                (uint8 plane)
// -- each output optional.  The resized [B,C,Ht,Wt] tensor (2.55 GB at 16 x 19 x 1024 x 2048) is never written.
//
// A block of 256 threads owns a tile of th x 64 label pixels (th = 16, 8 or 4) and stages the tile's source footprint -- at a
// 2x ratio about (th/2 + 2) x 34 source pixels of C floats -- in LDS as [row][pixel][C]; every source value then feeds its ~4
// label pixels (x 2: the log-sum-exp is two passes over the classes, the maximum first, and interpolates again rather than keep
// C values in registers) from LDS.  The host picks the largest th whose footprint fits beside the block's histogram in 64 KB;
// when none fits (strong downscaling; equal sizes with many classes) the same code reads the four taps straight from memory,
// served by the caches.  Pixel pitch in LDS is C: neighbouring lanes read the same or the neighbouring source pixel, and the
// class counts in use (19, 66) put a 32-lane group on distinct banks or on one broadcast address.
//
// Deterministic: block-private LDS histogram and one integer atomic per touched bin per block; the loss as one double pair per
// block, folded by se_finalize_kernel in a fixed order.  No float atomics.  The file is compiled with -ffp-contract=off.
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)
constexpr int SE_THREADS = 256, SE_TW = 64, SE_TH_MAX = 16, SE_TH_MIN = 4;
constexpr int SE_SCRATCH = 64;                       // bytes at the start of LDS for segsde_block_sum
constexpr size_t SE_LDS_MAX = 64 * 1024;             // scratch + histogram + tile

struct se_args {
  const float* logits;
  long sb, sc, sh, sw;             // element strides: batch, class, row, pixel
  const int64_t* labels;
  int64_t ignore;
  unsigned long long* hist;        // [C*C] or null
  double* part;                    // [blocks][2] or null
  unsigned char* ids;              // [B][Ht][Wt] or null
  int B, C, Hi, Wi, Ht, Wt;
  int th;                          // label rows of a tile
  int tile_floats;                 // LDS floats available for the staged footprint; 0: read the taps from memory
  int tiles_x, tiles_y;
};

// One label pixel.  p00..p11: the four taps' class-0 elements, cs: class stride.  The value of class c is the expression of
// resize_fwd_kernel; nll follows ce_nll of segmix.hip (x[t] - mx rounds at the size of the difference).
__device__ __forceinline__ void se_pixel(const float* p00, const float* p01, const float* p10, const float* p11, long cs, int C,
                                         const Lerp& lh, const Lerp& lw, int t, bool want_nll, int& arg, float& nll) {
  float best = 0.f, xt = 0.f;
  arg = 0;
  for (int c = 0; c < C; ++c) {
    const long o = c * cs;
    const float v = lh.l0 * (lw.l0 * p00[o] + lw.l1 * p01[o]) + lh.l1 * (lw.l0 * p10[o] + lw.l1 * p11[o]);
    if (c == 0) best = v;
    else if (v > best) { best = v; arg = c; }
    if (c == t) xt = v;
  }
  if (!want_nll) return;
  float se = 0.f;
  for (int c = 0; c < C; ++c) {
    const long o = c * cs;
    const float v = lh.l0 * (lw.l0 * p00[o] + lw.l1 * p01[o]) + lh.l1 * (lw.l0 * p10[o] + lw.l1 * p11[o]);
    se += expf(v - best);
  }
  nll = logf(se) - (xt - best);
}

template <bool STAGED>
__device__ __forceinline__ void se_tile(const se_args& A, const float* img, const float* tile, int r0, int c0, int afw, int ty0,
                                        int tx0, long lab0, unsigned* shist, double& num, double& den) {
  const int C = A.C;
  const int x = tx0 + (int)(threadIdx.x & 63);
  if (x >= A.Wt) return;
  const Lerp lw = lerp_src(x, A.Wi, A.Wt, 1);
  for (int yy = (int)(threadIdx.x >> 6); yy < A.th; yy += SE_THREADS / SE_TW) {
    const int y = ty0 + yy;
    if (y >= A.Ht) break;
    const long e = lab0 + (long)y * A.Wt + x;
    const int64_t t64 = A.labels[e];
    const bool in_range = t64 >= 0 && t64 < C;
    const bool want_nll = A.part && in_range && t64 != A.ignore;
    if (!A.ids && !(in_range && (A.hist || want_nll))) continue;
    const Lerp lh = lerp_src(y, A.Hi, A.Ht, 1);
    int arg;
    float nll = 0.f;
    if (STAGED) {
      const float* ra = tile + (long)(lh.i0 - r0) * afw * C;
      const float* rb = tile + (long)(lh.i1 - r0) * afw * C;
      const int xa = (lw.i0 - c0) * C, xb = (lw.i1 - c0) * C;
      se_pixel(ra + xa, ra + xb, rb + xa, rb + xb, 1, C, lh, lw, in_range ? (int)t64 : -1, want_nll, arg, nll);
    } else {
      const float* ra = img + lh.i0 * A.sh;
      const float* rb = img + lh.i1 * A.sh;
      const long xa = lw.i0 * A.sw, xb = lw.i1 * A.sw;
      se_pixel(ra + xa, ra + xb, rb + xa, rb + xb, A.sc, C, lh, lw, in_range ? (int)t64 : -1, want_nll, arg, nll);
    }
    if (A.ids) A.ids[e] = (unsigned char)arg;
    if (A.hist && in_range) atomicAdd(&shist[(int)t64 * C + arg], 1u);
    if (want_nll) { num += (double)nll; den += 1.0; }
  }
}

__global__ __launch_bounds__(SE_THREADS) void seg_eval_kernel(const se_args A) {
  SEGSDE_SMEM;
  double* red = reinterpret_cast<double*>(segsde_smem);
  unsigned* shist = reinterpret_cast<unsigned*>(segsde_smem + SE_SCRATCH);          // [C*C]
  float* tile = reinterpret_cast<float*>(shist + A.C * A.C);
  const int C = A.C, bins = C * C;
  if (A.hist) for (int i = threadIdx.x; i < bins; i += SE_THREADS) shist[i] = 0u;

  const int tiles = A.tiles_x * A.tiles_y;
  const int b = (int)(blockIdx.x / (unsigned)tiles), tl = (int)(blockIdx.x % (unsigned)tiles);
  const int ty0 = (tl / A.tiles_x) * A.th, tx0 = (tl % A.tiles_x) * SE_TW;
  const int ty1 = (ty0 + A.th < A.Ht ? ty0 + A.th : A.Ht) - 1;                        // last label row / pixel of the tile
  const int tx1 = (tx0 + SE_TW < A.Wt ? tx0 + SE_TW : A.Wt) - 1;
  // lerp_src is monotone in its destination index, so these four bound every tap of the tile
  const int r0 = lerp_src(ty0, A.Hi, A.Ht, 1).i0, r1 = lerp_src(ty1, A.Hi, A.Ht, 1).i1;
  const int c0 = lerp_src(tx0, A.Wi, A.Wt, 1).i0, c1 = lerp_src(tx1, A.Wi, A.Wt, 1).i1;
  const int afh = r1 - r0 + 1, afw = c1 - c0 + 1;
  const float* img = A.logits + b * A.sb;
  const bool staged = (long)afh * afw * C <= (long)A.tile_floats;                      // block-uniform

  if (staged) {
    const float* src = img + r0 * A.sh + c0 * A.sw;
    if (A.sc == 1 && A.sw == C) {                     // channels-last: a footprint row is one run of afw * C floats
      const int run = afw * C;
      for (int r = 0; r < afh; ++r) {
        const float* s = src + r * A.sh;
        float* d = tile + r * run;
        for (int e = threadIdx.x; e < run; e += SE_THREADS) d[e] = s[e];
      }
    } else {                                          // planes: lanes along the pixels, C loads in flight per lane
      for (int q = threadIdx.x; q < afh * afw; q += SE_THREADS) {
        const int r = q / afw, px = q - r * afw;
        const float* s = src + r * A.sh + px * A.sw;
        float* d = tile + (long)q * C;
        for (int c = 0; c < C; ++c) d[c] = s[c * A.sc];
      }
    }
  }
  __syncthreads();

  double num = 0.0, den = 0.0;
  const long lab0 = (long)b * A.Ht * A.Wt;
  if (staged) se_tile<true>(A, img, tile, r0, c0, afw, ty0, tx0, lab0, shist, num, den);
  else se_tile<false>(A, img, tile, r0, c0, afw, ty0, tx0, lab0, shist, num, den);

  __syncthreads();
  if (A.hist)
    for (int i = threadIdx.x; i < bins; i += SE_THREADS)
      if (shist[i]) atomicAdd(&A.hist[i], (unsigned long long)shist[i]);
  if (A.part) {
    const double a = segsde_block_sum(num, red);
    const double d = segsde_block_sum(den, red);
    if (threadIdx.x == 0) { A.part[2 * (long)blockIdx.x] = a; A.part[2 * (long)blockIdx.x + 1] = d; }
  }
}

// thread l adds the partials of blocks l, l + 256, ... in ascending order, then the fixed tree of segsde_block_sum
__global__ __launch_bounds__(SE_THREADS) void se_finalize_kernel(const double* part, long n, double* out) {
  SEGSDE_SMEM;
  double* red = reinterpret_cast<double*>(segsde_smem);
  double a = 0.0, d = 0.0;
  for (long i = threadIdx.x; i < n; i += SE_THREADS) { a += part[2 * i]; d += part[2 * i + 1]; }
  a = segsde_block_sum(a, red);
  d = segsde_block_sum(d, red);
  if (threadIdx.x == 0) { out[0] = a; out[1] = d; }
}

// source rows (pixels) that n consecutive destination indices can touch: i0 moves by at most floor(scale * (n - 1)) + 1 over
// them, i1 is one further
inline int se_span(int in, int out, int n) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const long s = (long)floor((double)scale * (double)(n - 1)) + 3;
  return (int)(s < in ? s : in);
}
inline size_t se_fixed_bytes(int C) { return (size_t)SE_SCRATCH + (size_t)C * C * sizeof(unsigned); }
inline bool se_supported(int C) { return se_fixed_bytes(C) + (size_t)4 * C * sizeof(float) <= SE_LDS_MAX; }   // a 2 x 2 footprint
// label rows per tile of the staged route and the LDS floats of its footprint; 0: direct reads
inline int se_plan(int C, int Hi, int Wi, int Ht, int Wt, int* tile_floats) {
  const int fw = se_span(Wi, Wt, Wt < SE_TW ? Wt : SE_TW);
  for (int th = SE_TH_MAX; th >= SE_TH_MIN; th >>= 1) {
    const size_t fl = (size_t)se_span(Hi, Ht, Ht < th ? Ht : th) * fw * C;
    if (se_fixed_bytes(C) + fl * sizeof(float) <= SE_LDS_MAX) { *tile_floats = (int)fl; return th; }
  }
  *tile_floats = 0;
  return 0;
}
inline long se_blocks(int B, int Ht, int Wt, int th) { return (long)B * segsde_cdiv(Ht, th) * segsde_cdiv(Wt, SE_TW); }
}  // namespace

extern "C" size_t segsde_seg_eval_workspace(int B, int Ht, int Wt) {
  if (B <= 0 || Ht <= 0 || Wt <= 0) return 0;
  return (size_t)se_blocks(B, Ht, Wt, SE_TH_MIN) * 2 * sizeof(double);       // the smallest tile: the most blocks
}

extern "C" int segsde_seg_eval_plan(int C, int Hi, int Wi, int Ht, int Wt) {
  if (C <= 0 || Hi <= 0 || Wi <= 0 || Ht <= 0 || Wt <= 0) return SEGSDE_ERR_SHAPE;
  if (!se_supported(C)) return SEGSDE_ERR_UNSUPPORTED;
  int fl;
  return se_plan(C, Hi, Wi, Ht, Wt, &fl);
}

extern "C" int segsde_seg_eval(const float* logits, long sb, long sc, long sh, long sw, int B, int C, int Hi, int Wi,
                               const int64_t* labels, int Ht, int Wt, int64_t ignore_index, unsigned long long* hist,
                               double* loss, unsigned char* ids, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !labels || (!hist && !loss && !ids) || (loss && !ws)) return SEGSDE_ERR_NULL;
  if (B <= 0 || C <= 0 || Hi <= 0 || Wi <= 0 || Ht <= 0 || Wt <= 0) return SEGSDE_ERR_SHAPE;
  if (!se_supported(C) || (ids && C > 256) || (long)Ht * Wt >= (1L << 32)) return SEGSDE_ERR_UNSUPPORTED;
  if (loss && (reinterpret_cast<uintptr_t>(ws) & 7)) return SEGSDE_ERR_UNSUPPORTED;
  if (loss && ws_bytes < segsde_seg_eval_workspace(B, Ht, Wt)) return SEGSDE_ERR_WORKSPACE;
  se_args A;
  A.logits = logits; A.sb = sb; A.sc = sc; A.sh = sh; A.sw = sw;
  A.labels = labels; A.ignore = ignore_index;
  A.hist = hist; A.part = loss ? static_cast<double*>(ws) : nullptr; A.ids = ids;
  A.B = B; A.C = C; A.Hi = Hi; A.Wi = Wi; A.Ht = Ht; A.Wt = Wt;
  A.th = se_plan(C, Hi, Wi, Ht, Wt, &A.tile_floats);
  if (A.th == 0) A.th = SE_TH_MAX;
  A.tiles_x = segsde_cdiv(Wt, SE_TW); A.tiles_y = segsde_cdiv(Ht, A.th);
  const long nb = se_blocks(B, Ht, Wt, A.th);
  if (nb > 0x7fffffffL) return SEGSDE_ERR_UNSUPPORTED;
  const size_t lds = se_fixed_bytes(C) + (size_t)A.tile_floats * sizeof(float);
  hipLaunchKernelGGL(seg_eval_kernel, dim3((unsigned)nb), dim3(SE_THREADS), lds, ST(stream), A);
  SEGSDE_CHECK_LAUNCH();
  if (loss) {
    hipLaunchKernelGGL(se_finalize_kernel, dim3(1), dim3(SE_THREADS), SE_SCRATCH, ST(stream), (const double*)A.part, nb, loss);
    SEGSDE_CHECK_LAUNCH();
  }
  return 0;
}
