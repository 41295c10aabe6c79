// Segmentation evaluation with test-time ensembling at LABEL resolution: K views of the same images (other input scales, a
// horizontally mirrored pass) are averaged as class probabilities on the label grid and scored like segeval.hip scores one view.
// For every label pixel, views in the given order:
//   the C logits of view k interpolated from its grid (lerp_src of segsde_common.h, align_corners=True: the arithmetic of
//   seg_eval_kernel and resize_fwd_kernel); a flipped view is read at source column w_k - 1 - i for tap column i, so the four
//   taps and their horizontal weights are those of the mirrored tensor;
//   p_k = softmax over the classes (the maximum first, then the sum of exp(z - max), then the terms again: three passes that
//   interpolate again from LDS rather than keep C values);
//   acc_c += (w_k / sum w) * p_k,c;
// then from acc: the argmax (strict >, the lowest index wins a tie), hist[C * label + argmax] += 1 where 0 <= label < C,
// loss sum += -log(max(acc[label], FLT_MIN)) and count += 1 where label != ignore_index and 0 <= label < C, ids[pixel] = argmax.
// Neither the resized logits nor the probabilities are written to memory: acc lives in LDS as [class][tile pixel].
//
// A block of 256 threads owns a tile of th x 64 label pixels (th = 16 .. 1; pixel q of the tile belongs to thread q % 256) and
// walks over the views.  Per view it stages the tile's source footprint in LDS as [row][pixel][C] -- mirrored while staging for
// a flipped view, so that the taps are read alike -- when the host's plan says it fits beside the histogram and the
// accumulator and holds no more source pixels than the tile reads taps (sn_footprint_floats); otherwise (strong downscaling,
// many classes) the four taps are read straight from memory through the caches.
// The plan (sn_plan) prefers, in this order, a tile of at least four rows (every thread owns a pixel) in 64 KB of LDS (more
// blocks per CU), then in the 160 KB a workgroup may have on gfx950, then the thinner tiles.
//
// One launch whatever K is, plus a one-block fold of the loss partials.  Deterministic: block-private LDS histogram and one
// integer atomic per touched bin per block; the loss as one double pair per block, folded in a fixed order.  No float atomics.
// The file is compiled with -ffp-contract=off.
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)
constexpr int SN_THREADS = 256, SN_TW = 64;
constexpr int SN_SCRATCH = 64;                        // bytes at the start of LDS for segsde_block_sum
constexpr size_t SN_LDS_SMALL = 64 * 1024;            // what every launch is granted
constexpr size_t SN_LDS_MAX = 160 * 1024;             // LDS of a CU, all of which one workgroup may ask for
constexpr int SN_MAX_VIEWS = SEGSDE_SEG_ENS_MAX_VIEWS;

struct sn_view {
  const float* logits;
  long sb, sc, sh, sw;             // element strides: batch, class, row, pixel
  int Hi, Wi;
  int flip;
  int staged;                      // the plan: stage the footprint in LDS (else read the taps from memory)
  float w;                         // w_k / sum w
  int pad_;
};

struct sn_args {
  sn_view v[SN_MAX_VIEWS];
  const int64_t* labels;           // null: only ids
  int64_t ignore;
  unsigned long long* hist;        // [C*C] or null
  double* part;                    // [blocks][2] or null
  unsigned char* ids;              // [B][Ht][Wt] or null
  int K, B, C, Ht, Wt;
  int th;                          // label rows of a tile
  int tile_floats;                 // LDS floats available for a staged footprint
  int tiles_x, tiles_y;
};

// interpolated logit of class offset o (the expression of resize_fwd_kernel and se_pixel)
__device__ __forceinline__ float sn_value(const float* p00, const float* p01, const float* p10, const float* p11, long o,
                                          const Lerp& lh, const Lerp& lw) {
  return lh.l0 * (lw.l0 * p00[o] + lw.l1 * p01[o]) + lh.l1 * (lw.l0 * p10[o] + lw.l1 * p11[o]);
}

// One label pixel of one view: acc[c * np] += w * softmax(z)[c].  p00..p11: the four taps' class-0 elements, cs: class stride.
__device__ __forceinline__ void sn_pixel(const float* p00, const float* p01, const float* p10, const float* p11, long cs, int C,
                                         const Lerp& lh, const Lerp& lw, float w, float* acc, int np) {
  float mx = sn_value(p00, p01, p10, p11, 0, lh, lw);
  for (int c = 1; c < C; ++c) {
    const float v = sn_value(p00, p01, p10, p11, c * cs, lh, lw);
    if (v > mx) mx = v;
  }
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(sn_value(p00, p01, p10, p11, c * cs, lh, lw) - mx);
  const float f = w * (1.f / se);
  for (int c = 0; c < C; ++c) acc[(long)c * np] += f * expf(sn_value(p00, p01, p10, p11, c * cs, lh, lw) - mx);
}

__global__ __launch_bounds__(SN_THREADS) void seg_ens_kernel(const sn_args A) {
  SEGSDE_SMEM;
  double* red = reinterpret_cast<double*>(segsde_smem);
  const int C = A.C, bins = C * C, np = A.th * SN_TW;
  unsigned* shist = reinterpret_cast<unsigned*>(segsde_smem + SN_SCRATCH);           // [C*C]
  float* acc = reinterpret_cast<float*>(shist + bins);                                // [C][np]
  float* tile = acc + (long)C * np;                                                   // [rows][pixels][C] of one view
  const int tid = (int)threadIdx.x;
  if (A.hist) for (int i = tid; i < bins; i += SN_THREADS) shist[i] = 0u;

  const int tiles = A.tiles_x * A.tiles_y;
  const int b = (int)(blockIdx.x / (unsigned)tiles), tl = (int)(blockIdx.x % (unsigned)tiles);
  const int ty0 = (tl / A.tiles_x) * A.th, tx0 = (tl % A.tiles_x) * SN_TW;
  const int ty1 = (ty0 + A.th < A.Ht ? ty0 + A.th : A.Ht) - 1;                        // last label row / pixel of the tile
  const int tx1 = (tx0 + SN_TW < A.Wt ? tx0 + SN_TW : A.Wt) - 1;
  const long lab0 = (long)b * A.Ht * A.Wt;
  const int x = tx0 + (tid & 63);

  // the thread's pixels q = tid, tid + 256, ...: one column, rows (tid >> 6) + 4 i.  Bit i of need: that pixel is evaluated.
  unsigned need = 0u;
  for (int q = tid, i = 0; q < np; q += SN_THREADS, ++i) {
    const int y = ty0 + (q >> 6);
    if (x >= A.Wt || y >= A.Ht) continue;
    bool on = A.ids != nullptr;
    if (!on && A.labels) {
      const int64_t t64 = A.labels[lab0 + (long)y * A.Wt + x];
      on = t64 >= 0 && t64 < C && (A.hist || (A.part && t64 != A.ignore));
    }
    if (on) {
      need |= 1u << i;
      for (int c = 0; c < C; ++c) acc[(long)c * np + q] = 0.f;
    }
  }

  for (int k = 0; k < A.K; ++k) {
    const sn_view& V = A.v[k];
    const float* img = V.logits + b * V.sb;
    // lerp_src is monotone in its destination index, so these four bound every tap of the tile (in the mirrored tensor's
    // columns for a flipped view)
    const int r0 = lerp_src(ty0, V.Hi, A.Ht, 1).i0, r1 = lerp_src(ty1, V.Hi, A.Ht, 1).i1;
    const int c0 = lerp_src(tx0, V.Wi, A.Wt, 1).i0, c1 = lerp_src(tx1, V.Wi, A.Wt, 1).i1;
    const int afh = r1 - r0 + 1, afw = c1 - c0 + 1;
    const bool staged = V.staged && (long)afh * afw * C <= (long)A.tile_floats;       // block-uniform
    if (staged) {
      __syncthreads();                                // the previous view's reads of the tile are done
      if (!V.flip && V.sc == 1 && V.sw == C) {        // channels-last: a footprint row is one run of afw * C floats
        const float* src = img + r0 * V.sh + c0 * V.sw;
        const int run = afw * C;
        for (int r = 0; r < afh; ++r) {
          const float* s = src + r * V.sh;
          float* d = tile + r * run;
          for (int e = tid; e < run; e += SN_THREADS) d[e] = s[e];
        }
      } else {                                        // lanes along the pixels, C loads in flight per lane
        for (int q = tid; q < afh * afw; q += SN_THREADS) {
          const int r = q / afw, px = q - r * afw;
          const int sx = V.flip ? V.Wi - 1 - (c0 + px) : c0 + px;
          const float* s = img + (r0 + r) * V.sh + sx * V.sw;
          float* d = tile + (long)q * C;
          for (int c = 0; c < C; ++c) d[c] = s[c * V.sc];
        }
      }
      __syncthreads();
    }
    if (!need) continue;
    const Lerp lw = lerp_src(x, V.Wi, A.Wt, 1);
    for (int q = tid, i = 0; q < np; q += SN_THREADS, ++i) {
      if (!((need >> i) & 1u)) continue;
      const Lerp lh = lerp_src(ty0 + (q >> 6), V.Hi, A.Ht, 1);
      if (staged) {
        const float* ra = tile + (long)(lh.i0 - r0) * afw * C;
        const float* rb = tile + (long)(lh.i1 - r0) * afw * C;
        const int xa = (lw.i0 - c0) * C, xb = (lw.i1 - c0) * C;
        sn_pixel(ra + xa, ra + xb, rb + xa, rb + xb, 1, C, lh, lw, V.w, acc + q, np);
      } else {
        const float* ra = img + lh.i0 * V.sh;
        const float* rb = img + lh.i1 * V.sh;
        const long xa = (V.flip ? V.Wi - 1 - lw.i0 : lw.i0) * V.sw, xb = (V.flip ? V.Wi - 1 - lw.i1 : lw.i1) * V.sw;
        sn_pixel(ra + xa, ra + xb, rb + xa, rb + xb, V.sc, C, lh, lw, V.w, acc + q, np);
      }
    }
  }
  __syncthreads();                                    // the histogram is zeroed

  double num = 0.0, den = 0.0;
  for (int q = tid, i = 0; q < np; q += SN_THREADS, ++i) {
    if (!((need >> i) & 1u)) continue;
    const long e = lab0 + (long)(ty0 + (q >> 6)) * A.Wt + x;
    const int64_t t64 = A.labels ? A.labels[e] : (int64_t)-1;
    const bool in_range = t64 >= 0 && t64 < C;
    float best = acc[q], at = 0.f;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      const float a = acc[(long)c * np + q];
      if (a > best) { best = a; arg = c; }
      if (c == (int)t64) at = a;
    }
    if (A.ids) A.ids[e] = (unsigned char)arg;
    if (A.hist && in_range) atomicAdd(&shist[(int)t64 * C + arg], 1u);
    if (A.part && in_range && t64 != A.ignore) {
      num += (double)(-logf(at > 1.17549435e-38f ? at : 1.17549435e-38f));
      den += 1.0;
    }
  }

  __syncthreads();
  if (A.hist)
    for (int i = tid; i < bins; i += SN_THREADS)
      if (shist[i]) atomicAdd(&A.hist[i], (unsigned long long)shist[i]);
  if (A.part) {
    const double a = segsde_block_sum(num, red);
    const double d = segsde_block_sum(den, red);
    if (tid == 0) { A.part[2 * (long)blockIdx.x] = a; A.part[2 * (long)blockIdx.x + 1] = d; }
  }
}

// thread l adds the partials of blocks l, l + 256, ... in ascending order, then the fixed tree of segsde_block_sum
__global__ __launch_bounds__(SN_THREADS) void sn_finalize_kernel(const double* part, long n, double* out) {
  SEGSDE_SMEM;
  double* red = reinterpret_cast<double*>(segsde_smem);
  double a = 0.0, d = 0.0;
  for (long i = threadIdx.x; i < n; i += SN_THREADS) { a += part[2 * i]; d += part[2 * i + 1]; }
  a = segsde_block_sum(a, red);
  d = segsde_block_sum(d, red);
  if (threadIdx.x == 0) { out[0] = a; out[1] = d; }
}

// source rows (pixels) that n consecutive destination indices can touch: i0 moves by at most floor(scale * (n - 1)) + 1 over
// them, i1 is one further
inline int sn_span(int in, int out, int n) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const long s = (long)floor((double)scale * (double)(n - 1)) + 3;
  return (int)(s < in ? s : in);
}
// histogram, accumulator and reduction scratch of a tile of th rows
inline size_t sn_fixed_bytes(int C, int th) {
  return (size_t)SN_SCRATCH + (size_t)C * C * sizeof(unsigned) + (size_t)th * SN_TW * C * sizeof(float);
}
// the one-row tile beside a 2 x 2 footprint
inline bool sn_supported(int C) { return sn_fixed_bytes(C, 1) + (size_t)4 * C * sizeof(float) <= SN_LDS_MAX; }
static_assert((size_t)SN_SCRATCH + (size_t)SEGSDE_SEG_ENS_MAX_CLASSES * SEGSDE_SEG_ENS_MAX_CLASSES * 4 +
              (size_t)(SN_TW + 4) * SEGSDE_SEG_ENS_MAX_CLASSES * 4 <= SN_LDS_MAX, "SEGSDE_SEG_ENS_MAX_CLASSES fits");
static_assert((size_t)SN_SCRATCH + (size_t)(SEGSDE_SEG_ENS_MAX_CLASSES + 1) * (SEGSDE_SEG_ENS_MAX_CLASSES + 1) * 4 +
              (size_t)(SN_TW + 4) * (SEGSDE_SEG_ENS_MAX_CLASSES + 1) * 4 > SN_LDS_MAX, "SEGSDE_SEG_ENS_MAX_CLASSES is the limit");

// LDS floats of a view's staged footprint; 0: not worth staging -- the footprint holds more source pixels than the tile reads
// taps in one pass over the classes (downscaling by more than about two per axis: no source value is read twice)
inline size_t sn_footprint_floats(int C, int Hi, int Wi, int Ht, int Wt, int th) {
  const int rows = Ht < th ? Ht : th, cols = Wt < SN_TW ? Wt : SN_TW;
  const size_t px = (size_t)sn_span(Hi, Ht, rows) * sn_span(Wi, Wt, cols);
  return px <= (size_t)4 * rows * cols ? px * C : 0;
}
inline bool sn_stages(size_t fixed, size_t fl, size_t budget) { return fl > 0 && fixed + fl * sizeof(float) <= budget; }

// The tile height and, per view, whether its footprint is staged.  Candidates in order of preference: tiles of >= 4 rows in
// 64 KB, then in 160 KB, then the thinner tiles likewise; the first that stages every view, else the first among those that
// stage the most.  tile_floats: the largest staged footprint.  0: no tile fits (sn_supported excludes that).
inline int sn_plan(int C, int K, const int* Hi, const int* Wi, int Ht, int Wt, int* staged, int* tile_floats) {
  static const int ths[2][3] = {{16, 8, 4}, {2, 1, 0}};
  int best_th = 0, best_n = -1;
  size_t best_budget = 0;
  for (int g = 0; g < 2; ++g)
    for (int t = 0; t < 2; ++t) {
      const size_t budget = t ? SN_LDS_MAX : SN_LDS_SMALL;
      for (int j = 0; j < 3 && ths[g][j]; ++j) {
        const int th = ths[g][j];
        const size_t fixed = sn_fixed_bytes(C, th);
        if (fixed > budget) continue;
        int n = 0;
        for (int k = 0; k < K; ++k) n += sn_stages(fixed, sn_footprint_floats(C, Hi[k], Wi[k], Ht, Wt, th), budget);
        if (n > best_n) { best_n = n; best_th = th; best_budget = budget; }
      }
    }
  *tile_floats = 0;
  if (!best_th) return 0;
  const size_t fixed = sn_fixed_bytes(C, best_th);
  for (int k = 0; k < K; ++k) {
    const size_t fl = sn_footprint_floats(C, Hi[k], Wi[k], Ht, Wt, best_th);
    staged[k] = sn_stages(fixed, fl, best_budget);
    if (staged[k] && (int)fl > *tile_floats) *tile_floats = (int)fl;
  }
  return best_th;
}
inline long sn_blocks(int B, int Ht, int Wt, int th) { return (long)B * segsde_cdiv(Ht, th) * segsde_cdiv(Wt, SN_TW); }

// the views that take part (weight > 0), in the given order; SEGSDE_ERR_* or their number
inline int sn_select(const segsde_seg_ens_view* views, int K, int* idx, double* total) {
  if (!views) return SEGSDE_ERR_NULL;
  if (K < 1 || K > SN_MAX_VIEWS) return SEGSDE_ERR_SHAPE;
  int n = 0;
  double sum = 0.0;
  for (int k = 0; k < K; ++k) {
    const float w = views[k].weight;
    if (!(w >= 0.f) || std::isinf(w) || views[k].Hi <= 0 || views[k].Wi <= 0) return SEGSDE_ERR_SHAPE;
    if (w > 0.f) { idx[n++] = k; sum += (double)w; }
  }
  if (n == 0) return SEGSDE_ERR_SHAPE;
  *total = sum;
  return n;
}
}  // namespace

extern "C" size_t segsde_seg_ens_workspace(int B, int Ht, int Wt) {
  if (B <= 0 || Ht <= 0 || Wt <= 0) return 0;
  return (size_t)sn_blocks(B, Ht, Wt, 1) * 2 * sizeof(double);               // the thinnest tile: the most blocks
}

extern "C" int segsde_seg_ens_plan(const segsde_seg_ens_view* views, int K, int C, int Ht, int Wt, int* staged) {
  int idx[SN_MAX_VIEWS], Hi[SN_MAX_VIEWS], Wi[SN_MAX_VIEWS], st[SN_MAX_VIEWS], fl;
  double total;
  const int n = sn_select(views, K, idx, &total);
  if (n < 0) return n;
  if (C <= 0 || Ht <= 0 || Wt <= 0) return SEGSDE_ERR_SHAPE;
  if (!sn_supported(C)) return SEGSDE_ERR_UNSUPPORTED;
  for (int j = 0; j < n; ++j) { Hi[j] = views[idx[j]].Hi; Wi[j] = views[idx[j]].Wi; }
  const int th = sn_plan(C, n, Hi, Wi, Ht, Wt, st, &fl);
  if (staged) {
    for (int k = 0; k < K; ++k) staged[k] = -1;                               // weight 0: the view is not read
    for (int j = 0; j < n; ++j) staged[idx[j]] = st[j];
  }
  return th;
}

extern "C" int segsde_seg_ens(const segsde_seg_ens_view* views, int K, int B, int C, const int64_t* labels, int Ht, int Wt,
                              int64_t ignore_index, unsigned long long* hist, double* loss, unsigned char* ids, void* ws,
                              size_t ws_bytes, void* stream) {
  if (!views || (!hist && !loss && !ids) || (loss && !ws) || (!labels && (hist || loss))) return SEGSDE_ERR_NULL;
  int idx[SN_MAX_VIEWS], Hi[SN_MAX_VIEWS], Wi[SN_MAX_VIEWS], st[SN_MAX_VIEWS];
  double total;
  const int n = sn_select(views, K, idx, &total);
  if (n < 0) return n;
  for (int j = 0; j < n; ++j)
    if (!views[idx[j]].logits) return SEGSDE_ERR_NULL;
  if (B <= 0 || C <= 0 || Ht <= 0 || Wt <= 0) return SEGSDE_ERR_SHAPE;
  if (!sn_supported(C) || (ids && C > 256) || (long)Ht * Wt >= (1L << 32)) return SEGSDE_ERR_UNSUPPORTED;
  if (loss && (reinterpret_cast<uintptr_t>(ws) & 7)) return SEGSDE_ERR_UNSUPPORTED;
  if (loss && ws_bytes < segsde_seg_ens_workspace(B, Ht, Wt)) return SEGSDE_ERR_WORKSPACE;
  sn_args A;
  for (int j = 0; j < n; ++j) { Hi[j] = views[idx[j]].Hi; Wi[j] = views[idx[j]].Wi; }
  A.th = sn_plan(C, n, Hi, Wi, Ht, Wt, st, &A.tile_floats);
  if (A.th == 0) return SEGSDE_ERR_UNSUPPORTED;
  for (int j = 0; j < SN_MAX_VIEWS; ++j) {
    sn_view& V = A.v[j];
    if (j >= n) { V = sn_view{nullptr, 0, 0, 0, 0, 1, 1, 0, 0, 0.f, 0}; continue; }
    const segsde_seg_ens_view& S = views[idx[j]];
    V.logits = S.logits; V.sb = S.sb; V.sc = S.sc; V.sh = S.sh; V.sw = S.sw;
    V.Hi = S.Hi; V.Wi = S.Wi; V.flip = S.flip ? 1 : 0; V.staged = st[j];
    V.w = (float)((double)S.weight / total);
    V.pad_ = 0;
  }
  A.labels = labels; A.ignore = ignore_index;
  A.hist = hist; A.part = loss ? static_cast<double*>(ws) : nullptr; A.ids = ids;
  A.K = n; A.B = B; A.C = C; A.Ht = Ht; A.Wt = Wt;
  A.tiles_x = segsde_cdiv(Wt, SN_TW); A.tiles_y = segsde_cdiv(Ht, A.th);
  const long nb = sn_blocks(B, Ht, Wt, A.th);
  if (nb > 0x7fffffffL) return SEGSDE_ERR_UNSUPPORTED;
  const size_t lds = sn_fixed_bytes(C, A.th) + (size_t)A.tile_floats * sizeof(float);
  if (lds > SN_LDS_SMALL) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(seg_ens_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return SEGSDE_ERR_UNSUPPORTED;                       // this device does not grant the workgroup that much LDS
  }
  hipLaunchKernelGGL(seg_ens_kernel, dim3((unsigned)nb), dim3(SN_THREADS), lds, ST(stream), A);
  SEGSDE_CHECK_LAUNCH();
  if (loss) {
    hipLaunchKernelGGL(sn_finalize_kernel, dim3(1), dim3(SN_THREADS), SN_SCRATCH, ST(stream), (const double*)A.part, nb, loss);
    SEGSDE_CHECK_LAUNCH();
  }
  return 0;
}
