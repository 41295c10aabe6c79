// Label selection (the reference's label_selection.py): the per-image uncertainty scores, the pooled depth-feature bank, its
// channel normalisation, the N x N distance matrix and the iterative farthest-point loop.  The arithmetic is small; what
// matters is that the discrete results are exact: the distance kernel uses the direct form sum (a - b)^2 (identical rows
// give exactly 0, the matrix is bitwise symmetric, the error does not grow with the norm of the features), the farthest-point
// kernel does comparisons only, and every sum is block partials + a finish pass in a fixed order (no float atomics).
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)

// ------------------------------------------------------------------------------------------------------------------ 1. scores
constexpr int SC_TH = 16, SC_TW = 64, SC_HALO = 3;                  // 1024 pixels per tile, 4 per thread
constexpr int SC_MH = SC_TH + 2 * SC_HALO, SC_MW = SC_TW + 2 * SC_HALO;
constexpr int SC_MAX_TILES = 256;                                   // grid.x cap: larger images take further passes
constexpr int SC_NQ = 1 + SEGSDE_LABELSEL_MAX_TYPES;

struct score_types { int t[SEGSDE_LABELSEL_MAX_TYPES]; };

__device__ __forceinline__ float inv_clamp(float d) { return fminf(fmaxf(1.f / d, 0.1f), 80.f); }

__device__ __forceinline__ float depth_error(int type, float dp, float ds) {
  switch (type) {
    case SEGSDE_DEPTH_ERR_ABS: return fabsf(dp - ds);
    case SEGSDE_DEPTH_ERR_ABS_INV_LOG: return fabsf(logf(inv_clamp(ds)) - logf(inv_clamp(dp)));
    case SEGSDE_DEPTH_ERR_ABS_INV: return fabsf(inv_clamp(ds) - inv_clamp(dp));
    case SEGSDE_DEPTH_ERR_SQ: { const float d = dp - ds; return d * d; }
    case SEGSDE_DEPTH_ERR_ABS_REL: return fabsf(dp - ds) / (ds + 0.1f);
    case SEGSDE_DEPTH_ERR_SQ_REL: { const float d = dp - ds; return (d * d) / (ds + 0.1f); }
    default: return fabsf(logf(1.f + dp) - logf(1.f + ds));
  }
}

// One block walks over tiles of 16 x 64 pixels of sample blockIdx.y.  Per tile: the mask disp_pseudo < 0.07 of the tile and a
// 3-pixel halo goes to LDS (zero outside the image), a horizontal 7-maximum into a second LDS plane, then every pixel takes the
// vertical 7-maximum (the 7x7 dilation), its class entropy straight from the strided logits, and the T error expressions.
// part: [B][gridDim.x][SC_NQ] doubles.
__global__ __launch_bounds__(256) void score_kernel(const float* logits, long sb, long sc, long sh, long sw, int C, int H, int W,
                                                    const float* disp_pred, const float* disp_pseudo, score_types types, int T,
                                                    int hcut, float log2c, float* entropy_map, float* error_maps, double* part) {
  SEGSDE_SMEM;
  double* red = reinterpret_cast<double*>(segsde_smem);                       // [4] block-sum scratch
  unsigned char* m0 = segsde_smem + 64;                                       // [SC_MH][SC_MW]
  unsigned char* m1 = m0 + SC_MH * SC_MW;                                     // [SC_MH][SC_TW] horizontal maxima
  const int b = blockIdx.y;
  const long HW = (long)H * W;
  const int tiles_x = (W + SC_TW - 1) / SC_TW, tiles_y = (H + SC_TH - 1) / SC_TH, ntiles = tiles_x * tiles_y;
  const float* lb = logits + b * sb;
  double acc[SC_NQ];
#pragma unroll
  for (int q = 0; q < SC_NQ; ++q) acc[q] = 0.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int y0 = (tile / tiles_x) * SC_TH, x0 = (tile % tiles_x) * SC_TW;
    if (T > 0) {
      __syncthreads();                                                        // the previous tile's readers are done
      for (int e = threadIdx.x; e < SC_MH * SC_MW; e += 256) {
        const int y = y0 - SC_HALO + e / SC_MW, x = x0 - SC_HALO + e % SC_MW;
        m0[e] = (y >= 0 && y < H && x >= 0 && x < W) ? (disp_pseudo[b * HW + (long)y * W + x] < 0.07f) : 0;
      }
      __syncthreads();
      for (int e = threadIdx.x; e < SC_MH * SC_TW; e += 256) {
        const unsigned char* r = m0 + (e / SC_TW) * SC_MW + e % SC_TW;
        m1[e] = r[0] | r[1] | r[2] | r[3] | r[4] | r[5] | r[6];
      }
      __syncthreads();
    }
    for (int e = threadIdx.x; e < SC_TH * SC_TW; e += 256) {
      const int ty = e / SC_TW, tx = e % SC_TW, y = y0 + ty, x = x0 + tx;
      if (y >= H || x >= W) continue;
      const long pix = (long)y * W + x;
      const float* lp = lb + y * sh + x * sw;
      float mx = lp[0];
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, lp[c * sc]);
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(lp[c * sc] - mx);
      float s = 0.f;
      for (int c = 0; c < C; ++c) {
        const float p = expf(lp[c * sc] - mx) / se;
        s += p * log2f(p + 1e-30f);
      }
      const float ent = -s / log2c;
      if (entropy_map) entropy_map[b * HW + pix] = ent;
      acc[0] += (double)ent;
      if (T > 0) {
        const unsigned char* col = m1 + ty * SC_TW + tx;
        unsigned char m = 0;
#pragma unroll
        for (int d = 0; d < 2 * SC_HALO + 1; ++d) m |= col[d * SC_TW];
        const float keep = 1.f - (float)m;
        const float dp = disp_pred[b * HW + pix], ds = disp_pseudo[b * HW + pix];
#pragma unroll
        for (int t = 0; t < SEGSDE_LABELSEL_MAX_TYPES; ++t) {
          if (t >= T) break;
          float v = depth_error(types.t[t], dp, ds) * keep;
          if (y >= hcut) v = 0.f;
          if (error_maps) error_maps[((long)b * T + t) * HW + pix] = v;
          acc[1 + t] += (double)v;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < SC_NQ; ++q) {
    if (q > T) break;                                                         // uniform: every thread leaves together
    const double r = segsde_block_sum(acc[q], red);
    if (threadIdx.x == 0) part[((long)b * gridDim.x + blockIdx.x) * SC_NQ + q] = r;
  }
}
__global__ __launch_bounds__(64) void score_finish_kernel(const double* part, int nblk, int T, double inv_n, float* table) {
  const int b = blockIdx.x, q = threadIdx.x;
  if (q > T) return;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) s += part[((long)b * nblk + i) * SC_NQ + q];
  table[(long)b * (1 + T) + q] = (float)(s * inv_n);
}
inline int score_blocks(int H, int W) {
  const long n = (long)((W + SC_TW - 1) / SC_TW) * ((H + SC_TH - 1) / SC_TH);
  return (int)(n > SC_MAX_TILES ? SC_MAX_TILES : n);
}

// ------------------------------------------------------------------------------------------------------------------ 2. pooling
__device__ __forceinline__ float pool_transform(float v, int transform) {
  if (transform == SEGSDE_POOL_NONE) return v;
  v = inv_clamp(v);
  return transform == SEGSDE_POOL_LOG_INV_CLAMP ? logf(v) : v;
}
// one thread per output element; the bins are at most a few hundred pixels.  max of the logdepth mode: log is monotone, so the
// maximum is taken over the clamped inverses (comparisons only) and logf is applied once to the winner
__global__ __launch_bounds__(256) void pool_kernel(const float* x, long sb, long sc, long sh, long sw, long total, int C, int H, int W,
                                                   int oh, int ow, int is_max, int transform, float* bank, long ld, long row0) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= total) return;
  const int oj = (int)(e % ow), oi = (int)((e / ow) % oh), c = (int)((e / ((long)ow * oh)) % C);
  const long b = e / ((long)ow * oh * C);
  const int ys = (int)(((long)oi * H) / oh), ye = (int)(((long)(oi + 1) * H + oh - 1) / oh);
  const int xs = (int)(((long)oj * W) / ow), xe = (int)(((long)(oj + 1) * W + ow - 1) / ow);
  const float* xp = x + b * sb + c * sc;
  const int each = (is_max && transform == SEGSDE_POOL_LOG_INV_CLAMP) ? SEGSDE_POOL_INV_CLAMP : transform;
  float r = is_max ? -INFINITY : 0.f;
  for (int y = ys; y < ye; ++y)
    for (int xx = xs; xx < xe; ++xx) {
      const float v = pool_transform(xp[y * sh + xx * sw], each);
      if (is_max) r = (v > r || v != v) ? v : r;      // NaN propagates as in torch
      else r += v;
    }
  if (!is_max) r = r / (float)((ye - ys) * (xe - xs));
  else if (each != transform) r = logf(r);
  bank[(row0 + b) * ld + ((long)c * oh + oi) * ow + oj] = r;
}

// ------------------------------------------------------------------------------------------------------------------ 3. normalise
constexpr int NM_MAX_BLK = 64, NM_PER_BLK = 4096;
inline int norm_blocks(long N, int P) {
  const long nb = (N * P + NM_PER_BLK - 1) / NM_PER_BLK;
  return (int)(nb < 1 ? 1 : (nb > NM_MAX_BLK ? NM_MAX_BLK : nb));
}
__device__ __forceinline__ double norm_fold(const double* p, int n) {      // the same order in every block
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += p[i];
  return s;
}
// pass 0: partial sums; pass 1: partial sums of squared deviations from the mean; pass 2: apply.  ws: [2][C][nblk] doubles
__global__ __launch_bounds__(256) void norm_kernel(float* bank, long ld, long N, int P, double* ws, int pass) {
  SEGSDE_SMEM;
  double* red = reinterpret_cast<double*>(segsde_smem);
  const int c = blockIdx.y, nblk = gridDim.x, C = gridDim.y;
  const long n = N * P;
  float* base = bank + (long)c * P;
  double* sum_part = ws + (long)c * nblk;
  double* dev_part = ws + ((long)C + c) * nblk;
  double mean_d = 0.0;
  float sd = 0.f;
  if (pass >= 1) mean_d = norm_fold(sum_part, nblk) / (double)n;
  if (pass == 2) sd = (float)sqrt(norm_fold(dev_part, nblk) / (double)(n - 1));
  const float mean = (float)mean_d;
  double acc = 0.0;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += (long)nblk * 256) {
    float* p = base + (e / P) * ld + e % P;
    const float v = *p;
    if (pass == 0) acc += (double)v;
    else if (pass == 1) { const double d = (double)v - mean_d; acc += d * d; }
    else *p = (v - mean) / sd;
  }
  if (pass < 2) {
    const double r = segsde_block_sum(acc, red);
    if (threadIdx.x == 0) (pass == 0 ? sum_part : dev_part)[blockIdx.x] = r;
  }
}

// ------------------------------------------------------------------------------------------------------------------ 4. distances
// A block of 256 threads forms a 64 x 64 tile of the matrix: rows i0.. against rows j0.. of the bank, D in chunks of 32 through LDS
// (k-major, so a thread's four rows are one 16-byte LDS read), each thread a 4 x 4 register block.  Chunks past D and rows past
// N are staged as zeros: (0 - 0)^2 adds exactly nothing.  Only tiles with bj >= bi compute; off-diagonal tiles write both halves.
constexpr int DT = 64, DK = 32, DLD = DT + 4;
template <int PNORM>
__global__ __launch_bounds__(256) void distance_kernel(const float* bank, long ld, int N, int D, const float* bias, float* out,
                                                       long ldo) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  SEGSDE_SMEM;
  float* As = reinterpret_cast<float*>(segsde_smem);                          // [DK][DLD]
  float* Bs = As + DK * DLD;
  const int i0 = bi * DT, j0 = bj * DT;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4], comp[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = comp[r][c] = 0.f;
  for (int k0 = 0; k0 < D; k0 += DK) {
    float part[4][4];                                                         // this chunk's 32 terms, summed in ascending k
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) part[r][c] = 0.f;
    __syncthreads();
    for (int e = threadIdx.x; e < DT * DK; e += 256) {
      const int r = e / DK, k = e % DK;
      const bool kin = k0 + k < D;
      As[k * DLD + r] = (kin && i0 + r < N) ? bank[(long)(i0 + r) * ld + k0 + k] : 0.f;
      Bs[k * DLD + r] = (kin && j0 + r < N) ? bank[(long)(j0 + r) * ld + k0 + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < DK; ++k) {
      const float4 a4 = *reinterpret_cast<const float4*>(As + k * DLD + ty * 4);
      const float4 b4 = *reinterpret_cast<const float4*>(Bs + k * DLD + tx * 4);
      const float a[4] = {a4.x, a4.y, a4.z, a4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float d = a[r] - bb[c];
          part[r][c] += PNORM == 2 ? d * d : fabsf(d);
        }
    }
    // the chunk sums join the total by a compensated (Kahan) addition: the error of the sum is that of 32 sequential
    // additions whatever D is (the sources are compiled without fast-math and with contraction off, so it stays)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float y = part[r][c] - comp[r][c];
        const float t = acc[r][c] + y;
        comp[r][c] = (t - acc[r][c]) - y;
        acc[r][c] = t;
      }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty * 4 + r, j = j0 + tx * 4 + c;
      if (i >= N || j >= N) continue;
      const float v = PNORM == 2 ? sqrtf(acc[r][c]) : acc[r][c];
      out[(long)i * ldo + j] = i == j ? 0.f : (bias ? v + bias[j] : v);
      if (bj != bi) out[(long)j * ldo + i] = bias ? v + bias[i] : v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ 4b. patch-wise distances
// The directed Chamfer distance between images: D[i][j] = (1/P) sum_a min_b || f[i,:,a] - f[j,:,b] ||.  The rows of the pair
// matrix are patches: patch a of image n is bank[n * ld + c * P + a], so a chunk of 32 channels of one image is already k-major.
// A block owns whole images on both sides: ipt = 64 / P of them (one when P > 64), R = ipt * P patch rows, and walks over the
// 64 x 64 sub-tiles of its R x R pair matrix (one for P <= 64, four for 64 < P <= 128).  Per sub-tile the pair sums are formed
// exactly as in distance_kernel (4 x 4 register block, chunks of 32 channels in ascending c, compensated addition of the chunk
// sums), parked in LDS over the dead operand chunks, and reduced to minima per (patch row, image on the other side):
//   Mrow[q][jj] = min over the patches b of image jj of d(q, b)      -> D[I][J]
//   Mcol[q][ii] = min over the patches a of image ii of d(a, q)      -> D[J][I]   (d is symmetric, D is not)
// A minimum that spans two sub-tiles is continued in LDS; the square root is taken once, when the last part has joined.  The
// comparison lets a NaN through from either side.  Rows past R and images past N are staged as zeros and never enter a minimum.
// Only blocks with bj >= bi compute.  The means run over a in ascending order: every result is a pure function of the inputs.
constexpr int PT = 64, PTLD = PT + 1;
inline int patch_ipt(int P) { return P >= PT ? 1 : PT / P; }
__device__ __forceinline__ float nan_min(float m, float v) { return (v < m || v != v) ? v : m; }

// the P minima of one image pair, added in ascending a; compensated, so that the error of the mean does not grow with P (a plain
// sum of 128 terms alone is 6 ulp off)
__device__ __forceinline__ float patch_mean(const float* m, int stride, int P) {
  float s = 0.f, comp = 0.f;
  for (int a = 0; a < P; ++a) {
    const float y = m[a * stride] - comp;
    const float t = s + y;
    comp = (t - s) - y;
    s = t;
  }
  return s;
}

template <int PNORM>
__global__ __launch_bounds__(256) void patch_distance_kernel(const float* bank, long ld, int N, int C, int P, int ipt,
                                                             const float* bias, float* out, long ldo) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  SEGSDE_SMEM;
  const int R = ipt * P, nsub = (R + PT - 1) / PT;
  float* As = reinterpret_cast<float*>(segsde_smem);                          // [DK][DLD]
  float* Bs = As + DK * DLD;
  float* Ts = As;                                                             // [PT][PTLD] pair sums, once the chunks are consumed
  float* Mrow = As + 2 * DK * DLD;                                            // [R][ipt]
  float* Mcol = Mrow + R * ipt;                                               // [R][ipt]
  static_assert(PT * PTLD <= 2 * DK * DLD && PT == DT, "the pair sums fit over the two operand chunks");
  const int img_i = bi * ipt, img_j = bj * ipt;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int sq = threadIdx.x % PT, sk = threadIdx.x / PT;                     // staging: patch row of the sub-tile, first channel
  for (int sr = 0; sr < nsub; ++sr)
    for (int sc = 0; sc < nsub; ++sc) {
      // staging: this thread's patch row of either side (the same in every chunk) and where its channel 0 lies in the bank
      const int qa = sr * PT + sq, qb = sc * PT + sq;
      const bool in_a = qa < R && img_i + qa / P < N, in_b = qb < R && img_j + qb / P < N;
      const long off_a = (long)(img_i + qa / P) * ld + qa % P, off_b = (long)(img_j + qb / P) * ld + qb % P;
      float acc[4][4], comp[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = comp[r][c] = 0.f;
      for (int k0 = 0; k0 < C; k0 += DK) {
        float part[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) part[r][c] = 0.f;
        __syncthreads();
        for (int k = sk; k < DK; k += 256 / PT) {                             // consecutive threads: consecutive patches of a channel
          const bool kin = k0 + k < C;
          const long ck = (long)(k0 + k) * P;
          As[k * DLD + sq] = (kin && in_a) ? bank[off_a + ck] : 0.f;
          Bs[k * DLD + sq] = (kin && in_b) ? bank[off_b + ck] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < DK; ++k) {
          const float4 a4 = *reinterpret_cast<const float4*>(As + k * DLD + ty * 4);
          const float4 b4 = *reinterpret_cast<const float4*>(Bs + k * DLD + tx * 4);
          const float a[4] = {a4.x, a4.y, a4.z, a4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float d = a[r] - bb[c];
              part[r][c] += PNORM == 2 ? d * d : fabsf(d);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {                                       // the compensated addition of distance_kernel
            const float y = part[r][c] - comp[r][c];
            const float t = acc[r][c] + y;
            comp[r][c] = (t - acc[r][c]) - y;
            acc[r][c] = t;
          }
      }
      __syncthreads();                                                        // the last chunk is consumed: Ts may cover it
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) Ts[(ty * 4 + r) * PTLD + tx * 4 + c] = acc[r][c];
      __syncthreads();
      for (int e = threadIdx.x; e < PT * ipt; e += 256) {                     // row minima: item (patch row a, image jj of J)
        const int a = e % PT, jj = e / PT, q = sr * PT + a;
        if (q >= R || img_i + q / P >= N || img_j + jj >= N) continue;
        const int lo = max(jj * P, sc * PT), hi = min(jj * P + P, sc * PT + PT);
        if (lo >= hi) continue;
        const int off = a * PTLD - sc * PT;
        float m = Ts[off + lo];
        for (int b = lo + 1; b < hi; ++b) m = nan_min(m, Ts[off + b]);
        float* dst = Mrow + q * ipt + jj;
        if (lo != jj * P) m = nan_min(m, *dst);                               // the part an earlier sub-tile left
        if (hi == jj * P + P && PNORM == 2) m = sqrtf(m);                     // the winner is known: one square root
        *dst = m;
      }
      if (bj != bi)
        for (int e = threadIdx.x; e < PT * ipt; e += 256) {                   // column minima: item (patch column b, image ii of I)
          const int b = e % PT, ii = e / PT, q = sc * PT + b;
          if (q >= R || img_j + q / P >= N || img_i + ii >= N) continue;
          const int lo = max(ii * P, sr * PT), hi = min(ii * P + P, sr * PT + PT);
          if (lo >= hi) continue;
          const int off = b - sr * PT * PTLD;
          float m = Ts[off + lo * PTLD];
          for (int a = lo + 1; a < hi; ++a) m = nan_min(m, Ts[off + a * PTLD]);
          float* dst = Mcol + q * ipt + ii;
          if (lo != ii * P) m = nan_min(m, *dst);
          if (hi == ii * P + P && PNORM == 2) m = sqrtf(m);
          *dst = m;
        }
    }
  __syncthreads();
  const float fP = (float)P;
  for (int e = threadIdx.x; e < ipt * ipt; e += 256) {
    const int ii = e / ipt, jj = e % ipt, i = img_i + ii, j = img_j + jj;
    if (i >= N || j >= N) continue;
    float v = patch_mean(Mrow + ii * P * ipt + jj, ipt, P) / fP;
    out[(long)i * ldo + j] = i == j ? 0.f : (bias ? v + bias[j] : v);
    if (bj != bi) {
      v = patch_mean(Mcol + jj * P * ipt + ii, ipt, P) / fP;
      out[(long)j * ldo + i] = bias ? v + bias[i] : v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ 5. farthest point
// One workgroup of 512 threads; thread t owns the columns t, t + 512, ...  LDS: mind[N] floats (the minimum over the current
// rows), flag[N] bytes (current sample or not), and a (value, index) pair per wave.
// Every loop is bounded by n_new, n_current or N; the threads meet at two barriers per step and three before the first.
constexpr int FP_THREADS = 512, FP_WAVES = FP_THREADS / 64;
inline size_t fps_lds(int N) { return 64 + ((size_t)N * 4 + 15) / 16 * 16 + (size_t)N; }
__global__ __launch_bounds__(FP_THREADS) void farthest_point_kernel(const float* dist, long ld, int N, const int* current, int n_current,
                                                                    const uint8_t* preselected, int n_new, int* out_idx,
                                                                    float* out_dist, int* out_count) {
  SEGSDE_SMEM;
  float* wval = reinterpret_cast<float*>(segsde_smem);                        // [FP_WAVES]
  int* widx = reinterpret_cast<int*>(segsde_smem + 32);                       // [FP_WAVES]
  float* mind = reinterpret_cast<float*>(segsde_smem + 64);                   // [N]
  unsigned char* flag = segsde_smem + 64 + ((size_t)N * 4 + 15) / 16 * 16;    // [N]
  const int tid = threadIdx.x;
  // which of this thread's (at most 64) columns take part in the preselection: one bit each in a register, so the LDS byte
  // holds the "current sample" bit alone and is only written between barriers that no reader crosses
  static_assert((SEGSDE_LABELSEL_FPS_MAX_N + FP_THREADS - 1) / FP_THREADS <= 64, "one bit per owned column");
  unsigned long long pre = 0;
  for (int j = tid, k = 0; j < N; j += FP_THREADS, ++k) {
    flag[j] = 0;
    if (!preselected || preselected[j]) pre |= 1ull << k;
  }
  __syncthreads();
  if (tid == 0)
    for (int c = 0; c < n_current; ++c) {
      const int ci = current[c];
      if ((unsigned)ci < (unsigned)N) flag[ci] = 1;                           // an index outside the matrix is ignored
    }
  __syncthreads();
  for (int j = tid, k = 0; j < N; j += FP_THREADS, ++k) {
    float m = INFINITY;
    if ((pre >> k) & 1) {
      for (int c = 0; c < n_current; ++c) {
        const int ci = current[c];
        if ((unsigned)ci < (unsigned)N) m = fminf(m, dist[(long)ci * ld + j]);
      }
    } else {
      m = 0.f;
    }
    mind[j] = m;
  }
  __syncthreads();
  int count = 0, fold = -1;                                                   // fold: the row recorded in the previous step
  for (int step = 0; step < n_new; ++step) {
    float bv = -INFINITY;
    int bidx = 0x7fffffff;
    for (int j = tid, k = 0; j < N; j += FP_THREADS, ++k) {
      float m = mind[j];
      if (fold >= 0) {
        const float v = ((pre >> k) & 1) ? dist[(long)fold * ld + j] : 0.f;
        m = fminf(m, v);
        mind[j] = m;
      }
      if (m > bv || bidx == 0x7fffffff) { bv = m; bidx = j; }                // ascending j: the first of equal values stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bidx, o);
      if (oi != 0x7fffffff && (bidx == 0x7fffffff || ov > bv || (ov == bv && oi < bidx))) { bv = ov; bidx = oi; }
    }
    if ((tid & 63) == 0) { wval[tid >> 6] = bv; widx[tid >> 6] = bidx; }
    __syncthreads();
    bv = wval[0]; bidx = widx[0];
    for (int w = 1; w < FP_WAVES; ++w) {
      const float ov = wval[w];
      const int oi = widx[w];
      if (oi != 0x7fffffff && (bidx == 0x7fffffff || ov > bv || (ov == bv && oi < bidx))) { bv = ov; bidx = oi; }
    }
    const bool stop = flag[bidx] != 0;
    __syncthreads();                                                          // everyone has read wval / widx / flag
    if (stop) break;
    if (tid == 0) { out_idx[count] = bidx; out_dist[count] = bv; flag[bidx] = 1; }      // next read: after the next step's first barrier
    ++count;
    fold = bidx;
  }
  if (tid == 0) out_count[0] = count;
}
}  // namespace

extern "C" size_t segsde_labelsel_score_workspace(int B, int H, int W, int T) {
  if (B <= 0 || H <= 0 || W <= 0 || T < 0) return 0;
  return (size_t)B * score_blocks(H, W) * SC_NQ * sizeof(double);
}

extern "C" int segsde_labelsel_score(const float* logits, long sb, long sc, long sh, long sw, int B, int C, int H, int W,
                                     const float* disp_pred, const float* disp_pseudo, const int* types, int T, float* table,
                                     float* entropy_map, float* error_maps, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !table || !ws) return SEGSDE_ERR_NULL;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || B > 65535 || T < 0 || T > SEGSDE_LABELSEL_MAX_TYPES) return SEGSDE_ERR_SHAPE;
  if (T > 0 && (!disp_pred || !disp_pseudo || !types)) return SEGSDE_ERR_NULL;
  if (C < 2 || C > SEGSDE_LABELSEL_MAX_CLASSES) return SEGSDE_ERR_UNSUPPORTED;
  score_types st = {};
  for (int t = 0; t < T; ++t) {
    if (types[t] < SEGSDE_DEPTH_ERR_ABS || types[t] > SEGSDE_DEPTH_ERR_ABS_LOG) return SEGSDE_ERR_SHAPE;
    st.t[t] = types[t];
  }
  if (ws_bytes < segsde_labelsel_score_workspace(B, H, W, T)) return SEGSDE_ERR_WORKSPACE;
  const int nb = score_blocks(H, W);
  const int hcut = (int)(0.87 * (double)H);
  const float log2c = (float)log2((double)C);
  hipLaunchKernelGGL(score_kernel, dim3(nb, B), dim3(256), 64 + SC_MH * SC_MW + SC_MH * SC_TW, ST(stream), logits, sb, sc, sh, sw, C,
                     H, W, disp_pred, disp_pseudo, st, T, hcut, log2c, entropy_map, T > 0 ? error_maps : nullptr, (double*)ws);
  SEGSDE_CHECK_LAUNCH();
  hipLaunchKernelGGL(score_finish_kernel, dim3(B), dim3(64), 0, ST(stream), (const double*)ws, nb, T, 1.0 / ((double)H * W), table);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_labelsel_pool(const float* x, long sb, long sc, long sh, long sw, int B, int C, int H, int W, int h, int is_max,
                                    int transform, float* bank, long ld_bank, long N, long row0, void* stream) {
  if (!x || !bank) return SEGSDE_ERR_NULL;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || h <= 0 || h > 16384 || N <= 0 || row0 < 0 || row0 + B > N ||
      ld_bank < (long)C * h * 2 * h)
    return SEGSDE_ERR_SHAPE;
  if (transform < SEGSDE_POOL_NONE || transform > SEGSDE_POOL_LOG_INV_CLAMP) return SEGSDE_ERR_UNSUPPORTED;
  const long total = (long)B * C * h * 2 * h;
  if ((total + 255) / 256 > 0x7fffffffL) return SEGSDE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST(stream), x, sb, sc, sh, sw, total, C, H, W,
                     h, 2 * h, is_max ? 1 : 0, transform, bank, ld_bank, row0);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t segsde_labelsel_normalize_workspace(long N, int C, int P) {
  if (N <= 0 || C <= 0 || P <= 0) return 0;
  return (size_t)2 * C * norm_blocks(N, P) * sizeof(double);
}

extern "C" int segsde_labelsel_normalize(float* bank, long ld, long N, int C, int P, void* ws, size_t ws_bytes, void* stream) {
  if (!bank || !ws) return SEGSDE_ERR_NULL;
  if (N <= 0 || C <= 0 || P <= 0 || C > 65535 || ld < (long)C * P) return SEGSDE_ERR_SHAPE;
  if (ws_bytes < segsde_labelsel_normalize_workspace(N, C, P)) return SEGSDE_ERR_WORKSPACE;
  const dim3 grid(norm_blocks(N, P), C);
  for (int pass = 0; pass < 3; ++pass) {
    hipLaunchKernelGGL(norm_kernel, grid, dim3(256), 64, ST(stream), bank, ld, N, P, (double*)ws, pass);
    SEGSDE_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int segsde_labelsel_distance(const float* bank, long ld, int N, int D, int p, const float* bias, float* out, long ldo,
                                        void* stream) {
  if (!bank || !out) return SEGSDE_ERR_NULL;
  if (N <= 0 || D <= 0 || ld < D || ldo < N) return SEGSDE_ERR_SHAPE;
  if (p != 1 && p != 2) return SEGSDE_ERR_UNSUPPORTED;
  const int nt = (N + DT - 1) / DT;
  if (nt > 65535) return SEGSDE_ERR_UNSUPPORTED;
  const size_t smem = (size_t)2 * DK * DLD * sizeof(float);
  if (p == 2)
    hipLaunchKernelGGL(distance_kernel<2>, dim3(nt, nt), dim3(256), smem, ST(stream), bank, ld, N, D, bias, out, ldo);
  else
    hipLaunchKernelGGL(distance_kernel<1>, dim3(nt, nt), dim3(256), smem, ST(stream), bank, ld, N, D, bias, out, ldo);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_labelsel_patch_distance(const float* bank, long ld, int N, int C, int P, int p, const float* bias, float* out,
                                              long ldo, void* stream) {
  if (!bank || !out) return SEGSDE_ERR_NULL;
  if (N <= 0 || C <= 0) return SEGSDE_ERR_SHAPE;
  if ((p != 1 && p != 2) || P < 1 || P > SEGSDE_LABELSEL_PATCH_MAX_P || (long)N * P >= (1L << 31)) return SEGSDE_ERR_UNSUPPORTED;
  if (ld < (long)C * P || ldo < N) return SEGSDE_ERR_SHAPE;
  const int ipt = patch_ipt(P);
  const int ng = (N + ipt - 1) / ipt;
  if (ng > 65535) return SEGSDE_ERR_UNSUPPORTED;                              // more image groups than a grid dimension takes
  const size_t smem = ((size_t)2 * DK * DLD + (size_t)2 * ipt * P * ipt) * sizeof(float);      // at most 50 176 B (P = 1)
  if (p == 2)
    hipLaunchKernelGGL(patch_distance_kernel<2>, dim3(ng, ng), dim3(256), smem, ST(stream), bank, ld, N, C, P, ipt, bias, out, ldo);
  else
    hipLaunchKernelGGL(patch_distance_kernel<1>, dim3(ng, ng), dim3(256), smem, ST(stream), bank, ld, N, C, P, ipt, bias, out, ldo);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_labelsel_farthest_point(const float* dist, long ld, int N, const int* current, int n_current,
                                              const uint8_t* preselected, int n_new, int* out_idx, float* out_dist, int* out_count,
                                              void* stream) {
  if (!dist || !current || !out_idx || !out_dist || !out_count) return SEGSDE_ERR_NULL;
  if (N <= 0 || n_current <= 0 || n_new < 0 || ld < N) return SEGSDE_ERR_SHAPE;
  if (N > SEGSDE_LABELSEL_FPS_MAX_N) return SEGSDE_ERR_UNSUPPORTED;
  const size_t smem = fps_lds(N);
  if (smem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(farthest_point_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)smem);
    if (e != hipSuccess) return SEGSDE_ERR_UNSUPPORTED;                       // this device does not grant the workgroup that much LDS
  }
  hipLaunchKernelGGL(farthest_point_kernel, dim3(1), dim3(FP_THREADS), smem, ST(stream), dist, ld, N, current, n_current, preselected,
                     n_new, out_idx, out_dist, out_count);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}
