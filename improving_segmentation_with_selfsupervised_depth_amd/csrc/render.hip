// Output side of a forward pass (inference.py:84-116 and the image block of Trainer.validate, train.py:904-923 of the reference):
// the uint8 images the reference writes into its files, made on the device so that one copy per batch leaves it.
//   render_labels      argmax over the class planes (or a given id map) -> palette colour, uint8 [B,H,W,3] (+ the id plane)
//   render_unit_image  float image in [0,1] -> uint8 [B,H,W,C] by save_image's  x.mul(255).add_(0.5).clamp_(0,255)  + truncation
//   colorize           _colorize (train.py:137-151) with max_percentile == 100: per-image min / max, index, table lookup
// All three are HBM-bound and read their input once.  Element and byte offsets are 64-bit throughout (16 x 19 x 1024 x 2048 fp32
// logits are 2.5 GB).
//
// Byte output.  The pixels of a launch are numbered flat over the whole batch, e = b * H * W + y * W + x, and cut into tiles of
// RENDER_TILE = 1024: a tile's output starts at byte tile * 1024 * C of a dense [B,H,W,C] tensor, which is dword aligned whatever
// the row pitch (W * C bytes) and the image pitch are -- 5 x 7 x 3 = 105 bytes per image is fine.  A thread takes the pixels
// t, t + 256, t + 512, t + 768 of the tile (dword loads of consecutive lanes are consecutive for NCHW sources), puts its bytes
// into an LDS image of the tile's output, and after a barrier the block writes that image with dword stores of consecutive
// lanes; only the last, partial tile of a launch ends in up to three single-byte stores.  The output base must be dword aligned.
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)
constexpr int RENDER_TILE = 1024;
constexpr int RENDER_PER_THREAD = RENDER_TILE / 256;

inline int tile_blocks(long total) {
  long nb = (total + RENDER_TILE - 1) / RENDER_TILE;
  return (int)(nb < 1 ? 1 : (nb > 4096 ? 4096 : nb));
}

// element offset of flat pixel e in a [B,*,H,W] view with element strides (sb, sh, sw); channel 0.  b0 is the image of the
// tile's first pixel, worked out once per tile: a pixel divides only where its tile runs into the next image, and -- with
// rows_dense, sh == W * sw, which dense NCHW, channels-last and channel slices all are -- not at all inside an image.
__device__ __forceinline__ long pixel_offset(long e, long b0, long HW, int W, long sb, long sh, long sw, int rows_dense) {
  long b = b0, p = e - b0 * HW;
  if (p >= HW) { b = e / HW; p = e - b * HW; }
  if (rows_dense) return b * sb + p * sw;
  const long y = p / W, x = p - y * W;
  return b * sb + y * sh + x * sw;
}

// the block's LDS image of `nbytes` output bytes -> dst (dword aligned): dwords by consecutive lanes, then the tail bytes
__device__ __forceinline__ void flush_tile(const unsigned char* stage, uint8_t* dst, int nbytes) {
  const int nd = nbytes >> 2;
  const unsigned* s4 = reinterpret_cast<const unsigned*>(stage);
  unsigned* d4 = reinterpret_cast<unsigned*>(dst);
  for (int i = threadIdx.x; i < nd; i += 256) d4[i] = s4[i];
  const int rest = nbytes - (nd << 2);
  if ((int)threadIdx.x < rest) dst[(nd << 2) + threadIdx.x] = stage[(nd << 2) + threadIdx.x];
}

// colour and saturated id of class / map value v for pixel q of the tile, into the tile's LDS images
__device__ __forceinline__ void emit_label(unsigned long long v, int q, const unsigned char* s_pal, int n, int zero_unmapped,
                                           unsigned char* s_rgb, unsigned char* s_id) {
  const unsigned char sat = (unsigned char)(v > 255ull ? 255ull : v);
  unsigned char r, g, b;
  if (v < (unsigned long long)n) {
    r = s_pal[3 * (int)v]; g = s_pal[3 * (int)v + 1]; b = s_pal[3 * (int)v + 2];
  } else {
    r = g = b = zero_unmapped ? (unsigned char)0 : sat;      // keep: the id in all three channels, clamped by save_image
  }
  s_rgb[3 * q] = r; s_rgb[3 * q + 1] = g; s_rgb[3 * q + 2] = b;
  s_id[q] = sat;
}

// LDS: [tile rgb 3072 B][tile ids 1024 B][palette 768 B][pixel offsets 2048 B][rows S (C|1) floats]; the last two only with S > 0.
// S > 0 (channel-contiguous logits, sc == 1: the package's own NHWC activations seen as NCHW): the C floats of a pixel lie
// together, so a thread scanning its own pixel would touch 4 bytes of every cache line per load.  Instead the block copies the
// rows of S pixels at a time into LDS with consecutive lanes on consecutive dwords (the pixel offsets are worked out once per
// pixel and kept in LDS; the copy loop walks (pixel, class) incrementally, no division), and thread t scans row t there (row
// pitch C|1 floats: odd, conflict-free).
template <typename IdT>
__global__ __launch_bounds__(256) void render_labels_kernel(const float* logits, long sb, long sc, long sh, long sw,
                                                            const IdT* ids, long HW, int W, long total, int C, int S,
                                                            const uint8_t* palette, int n, int zero_unmapped, uint8_t* rgb,
                                                            uint8_t* ids_out) {
  SEGSDE_SMEM;
  const int rows_dense = sh == (long)W * sw;
  unsigned char* s_rgb = segsde_smem;
  unsigned char* s_id = segsde_smem + 3 * RENDER_TILE;
  unsigned char* s_pal = segsde_smem + 4 * RENDER_TILE;
  long* s_off = reinterpret_cast<long*>(segsde_smem + 4 * RENDER_TILE + 3 * SEGSDE_RENDER_MAX_COLORS);
  float* s_x = reinterpret_cast<float*>(segsde_smem + 4 * RENDER_TILE + 3 * SEGSDE_RENDER_MAX_COLORS + 8 * 256);
  const int t = threadIdx.x;
  for (int i = t; i < 3 * n; i += 256) s_pal[i] = palette[i];
  const long ntiles = (total + RENDER_TILE - 1) / RENDER_TILE;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long e0 = tile * RENDER_TILE;
    const int np = (int)(total - e0 < RENDER_TILE ? total - e0 : RENDER_TILE);
    const long b0 = e0 / HW;
    __syncthreads();      // the palette is staged; the previous tile's image has been written out
    if (logits && S > 0) {
      const int Cp = C | 1;
      const int dp = 256 / C, dc = 256 - dp * C;
      for (int q0 = 0; q0 < np; q0 += S) {
        const int ns = np - q0 < S ? np - q0 : S;
        __syncthreads();      // the rows of the previous group have been scanned
        if (t < ns) s_off[t] = pixel_offset(e0 + q0 + t, b0, HW, W, sb, sh, sw, rows_dense);
        __syncthreads();
        int pix = t / C, c = t - pix * C;
        for (int i = t; i < ns * C; i += 4 * 256) {      // four loads in flight per thread, then their LDS stores
          float v[4];
          int d[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            d[u] = i + 256 * u < ns * C ? pix * Cp + c : -1;
            v[u] = d[u] >= 0 ? logits[s_off[pix] + c] : 0.f;
            pix += dp; c += dc;
            if (c >= C) { c -= C; ++pix; }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (d[u] >= 0) s_x[d[u]] = v[u];
        }
        __syncthreads();
        if (t < ns) {
          const float* row = s_x + t * Cp;
          float best = row[0];
          int arg = 0;
          for (int k = 1; k < C; ++k) {
            const float x = row[k];
            if (x > best) { best = x; arg = k; }
          }
          emit_label((unsigned long long)arg, q0 + t, s_pal, n, zero_unmapped, s_rgb, s_id);
        }
      }
    } else {
      unsigned long long v[RENDER_PER_THREAD];
      if (logits) {
        const float* src[RENDER_PER_THREAD];
        float best[RENDER_PER_THREAD];
#pragma unroll
        for (int k = 0; k < RENDER_PER_THREAD; ++k) {
          const int q = t + 256 * k;
          src[k] = logits + pixel_offset(e0 + (q < np ? q : 0), b0, HW, W, sb, sh, sw, rows_dense);
          best[k] = src[k][0];
          v[k] = 0;
        }
        for (int c = 1; c < C; ++c) {
#pragma unroll
          for (int k = 0; k < RENDER_PER_THREAD; ++k) {
            const float x = src[k][(long)c * sc];
            if (x > best[k]) { best[k] = x; v[k] = (unsigned long long)c; }      // strict: the first maximum wins (torch.max on the CPU)
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < RENDER_PER_THREAD; ++k) {
          const int q = t + 256 * k;
          v[k] = (unsigned long long)ids[e0 + (q < np ? q : 0)];      // ids are taken as non-negative
        }
      }
#pragma unroll
      for (int k = 0; k < RENDER_PER_THREAD; ++k) emit_label(v[k], t + 256 * k, s_pal, n, zero_unmapped, s_rgb, s_id);
    }
    __syncthreads();
    flush_tile(s_rgb, rgb + 3 * e0, 3 * np);
    if (ids_out) flush_tile(s_id, ids_out + e0, np);
  }
}

// save_image's arithmetic on one value: two separately rounded fp32 operations, clamp, truncation; NaN -> 0
__device__ __forceinline__ unsigned char unit_to_byte(float x) {
#pragma clang fp contract(off)
  float t = x * 255.0f;
  t = t + 0.5f;
  if (t != t) return 0;
  t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
  return (unsigned char)(int)t;
}

// LDS: [tile bytes 1024 C]
__global__ __launch_bounds__(256) void render_unit_image_kernel(const float* x, long sb, long sc, long sh, long sw, long HW, int W,
                                                                long total, int C, uint8_t* out) {
  SEGSDE_SMEM;
  const int rows_dense = sh == (long)W * sw;
  unsigned char* stage = segsde_smem;
  const long ntiles = (total + RENDER_TILE - 1) / RENDER_TILE;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long e0 = tile * RENDER_TILE;
    const int np = (int)(total - e0 < RENDER_TILE ? total - e0 : RENDER_TILE);
    const long b0 = e0 / HW;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RENDER_PER_THREAD; ++k) {
      const int q = threadIdx.x + 256 * k;
      const float* src = x + pixel_offset(e0 + (q < np ? q : 0), b0, HW, W, sb, sh, sw, rows_dense);
      for (int c = 0; c < C; ++c) stage[q * C + c] = unit_to_byte(src[(long)c * sc]);
    }
    __syncthreads();
    flush_tile(stage, out + (long)C * e0, C * np);
  }
}

// numpy's minimum / maximum: a NaN operand wins
__device__ __forceinline__ float np_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ float np_max(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

inline int colorize_blocks(long HW) { long nb = (HW + 1023) / 1024; return (int)(nb < 1 ? 1 : (nb > 256 ? 256 : nb)); }

// pass 1: block partials of np.min / np.max per image, part [B][nblk][2]
__global__ __launch_bounds__(256) void colorize_minmax_kernel(const float* x, long HW, float* part) {
  SEGSDE_SMEM;
  float* sh = reinterpret_cast<float*>(segsde_smem);      // [2][4]
  const int b = blockIdx.y;
  const float* xb = x + (long)b * HW;
  // four loads in flight per thread, each with its own running pair (min / max are order-independent, NaN included)
  float m0 = INFINITY, m1 = INFINITY, m2 = INFINITY, m3 = INFINITY, x0 = -INFINITY, x1 = -INFINITY, x2 = -INFINITY, x3 = -INFINITY;
  const long step = (long)gridDim.x * 256;
  long e = blockIdx.x * 256L + threadIdx.x;
  for (; e + 3 * step < HW; e += 4 * step) {
    const float a = xb[e], b1 = xb[e + step], c = xb[e + 2 * step], d = xb[e + 3 * step];
    m0 = np_min(m0, a); x0 = np_max(x0, a); m1 = np_min(m1, b1); x1 = np_max(x1, b1);
    m2 = np_min(m2, c); x2 = np_max(x2, c); m3 = np_min(m3, d); x3 = np_max(x3, d);
  }
  for (; e < HW; e += step) { const float a = xb[e]; m0 = np_min(m0, a); x0 = np_max(x0, a); }
  float mn = np_min(np_min(m0, m1), np_min(m2, m3)), mx = np_max(np_max(x0, x1), np_max(x2, x3));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = np_min(mn, __shfl_xor(mn, o)); mx = np_max(mx, __shfl_xor(mx, o)); }
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = mn; sh[4 + (threadIdx.x >> 6)] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { mn = np_min(mn, sh[i]); mx = np_max(mx, sh[4 + i]); }
    part[((long)b * gridDim.x + blockIdx.x) * 2] = mn;
    part[((long)b * gridDim.x + blockIdx.x) * 2 + 1] = mx;
  }
}

// pass 2: every block folds its image's partials, then one thread per OUTPUT float (pixel j / 3, channel j % 3: the three lanes
// of a pixel read the same input dword, the stores of consecutive lanes are consecutive).  LDS: [8 floats][table 3 (N + 3) floats]
__global__ __launch_bounds__(256) void colorize_apply_kernel(const float* x, long HW, const float* part, int nblk, const float* lut,
                                                             int N, int mask_zero, float* out) {
#pragma clang fp contract(off)
  SEGSDE_SMEM;
  float* sh = reinterpret_cast<float*>(segsde_smem);
  float* s_lut = sh + 8;
  for (int i = threadIdx.x; i < 3 * (N + 3); i += 256) s_lut[i] = lut[i];
  const int b = blockIdx.y;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < nblk; i += 256) {
    mn = np_min(mn, part[((long)b * nblk + i) * 2]); mx = np_max(mx, part[((long)b * nblk + i) * 2 + 1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = np_min(mn, __shfl_xor(mn, o)); mx = np_max(mx, __shfl_xor(mx, o)); }
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = mn; sh[4 + (threadIdx.x >> 6)] = mx; }
  __syncthreads();
  const float vmin = np_min(np_min(sh[0], sh[1]), np_min(sh[2], sh[3]));
  const float vmax = np_max(np_max(sh[4], sh[5]), np_max(sh[6], sh[7]));
  const float fN = (float)N;
  const float* xb = x + (long)b * HW;
  float* ob = out + 3 * (long)b * HW;
  const long n3 = 3 * HW;
  for (long j = blockIdx.x * 256L + threadIdx.x; j < n3; j += (long)gridDim.x * 256) {
    const long p = j / 3;
    const int ch = (int)(j - 3 * p);
    const float v = xb[p];
    const float q = np_min(np_max(v, vmin), vmax) / vmax;      // np.clip(img, vmin, vmax) / vmax; 0 / 0 = NaN -> the bad colour
    const float s = q * fN;
    int idx;
    if (s == fN) idx = N - 1;
    else if (s < 0.0f) idx = N;            // under
    else if (s > fN) idx = N + 1;          // over
    else if (s != s) idx = N + 2;          // bad
    else idx = (int)s;
    ob[j] = (mask_zero && v <= 0.0f) ? 1.0f : s_lut[3 * idx + ch];
  }
}
}  // namespace

extern "C" int segsde_render_labels(const float* logits, long sb, long sc, long sh, long sw, const void* ids, int ids_dtype, int B,
                                    int C, int H, int W, const uint8_t* palette, int n, int unmapped, uint8_t* rgb,
                                    uint8_t* ids_out, void* stream) {
  if ((!logits && !ids) || !palette || !rgb) return SEGSDE_ERR_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || n <= 0 || (logits && C <= 0)) return SEGSDE_ERR_SHAPE;
  if (n > SEGSDE_RENDER_MAX_COLORS) return SEGSDE_ERR_UNSUPPORTED;
  if (unmapped != SEGSDE_RENDER_UNMAPPED_KEEP && unmapped != SEGSDE_RENDER_UNMAPPED_ZERO) return SEGSDE_ERR_UNSUPPORTED;
  if (!logits && ids_dtype != SEGSDE_DTYPE_I64 && ids_dtype != SEGSDE_DTYPE_U8) return SEGSDE_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(ids_out)) & 3) return SEGSDE_ERR_UNSUPPORTED;
  const long HW = (long)H * W, total = (long)B * HW;
  // rows staged in LDS for channel-contiguous logits: the largest group of pixels whose rows fit 48 KB (C <= 383), else none
  int S = 0;
  if (logits && sc == 1 && C > 1)
    for (S = 256; S >= 32 && (size_t)S * (C | 1) * sizeof(float) > 48 * 1024; S >>= 1) {}
  if (S < 32) S = 0;
  const size_t lds = 4 * RENDER_TILE + 3 * SEGSDE_RENDER_MAX_COLORS + (S ? 8 * 256 + (size_t)S * (C | 1) * sizeof(float) : 0);
  const dim3 grid(tile_blocks(total)), block(256);
  const int zero = unmapped == SEGSDE_RENDER_UNMAPPED_ZERO;
  if (logits || ids_dtype == SEGSDE_DTYPE_I64)
    hipLaunchKernelGGL(render_labels_kernel<int64_t>, grid, block, lds, ST(stream), logits, sb, sc, sh, sw,
                       logits ? nullptr : (const int64_t*)ids, HW, W, total, C, S, palette, n, zero, rgb, ids_out);
  else
    hipLaunchKernelGGL(render_labels_kernel<uint8_t>, grid, block, lds, ST(stream), logits, sb, sc, sh, sw, (const uint8_t*)ids, HW,
                       W, total, C, S, palette, n, zero, rgb, ids_out);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_render_unit_image(const float* x, long sb, long sc, long sh, long sw, int B, int C, int H, int W,
                                        uint8_t* out, void* stream) {
  if (!x || !out) return SEGSDE_ERR_NULL;
  if (B <= 0 || H <= 0 || W <= 0) return SEGSDE_ERR_SHAPE;
  if (C != 1 && C != 3) return SEGSDE_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(out) & 3) return SEGSDE_ERR_UNSUPPORTED;
  const long HW = (long)H * W, total = (long)B * HW;
  hipLaunchKernelGGL(render_unit_image_kernel, dim3(tile_blocks(total)), dim3(256), (size_t)RENDER_TILE * C, ST(stream), x, sb, sc,
                     sh, sw, HW, W, total, C, out);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t segsde_colorize_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * colorize_blocks((long)H * W) * 2 * sizeof(float);
}

extern "C" int segsde_colorize(const float* img, int B, int H, int W, const float* lut, int N, int mask_zero, float* out, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!img || !lut || !out || !ws) return SEGSDE_ERR_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || N <= 0) return SEGSDE_ERR_SHAPE;
  if (N > SEGSDE_COLORIZE_MAX_N) return SEGSDE_ERR_UNSUPPORTED;
  if (ws_bytes < segsde_colorize_workspace(B, H, W)) return SEGSDE_ERR_WORKSPACE;
  const long HW = (long)H * W;
  const int nb = colorize_blocks(HW);
  hipLaunchKernelGGL(colorize_minmax_kernel, dim3(nb, B), dim3(256), 64, ST(stream), img, HW, (float*)ws);
  SEGSDE_CHECK_LAUNCH();
  long nb2 = (3 * HW + 1023) / 1024;
  nb2 = nb2 < 1 ? 1 : (nb2 > 1024 ? 1024 : nb2);
  hipLaunchKernelGGL(colorize_apply_kernel, dim3((unsigned)nb2, B), dim3(256), (size_t)(8 + 3 * (N + 3)) * sizeof(float), ST(stream), img,
                     HW, (const float*)ws, nb, lut, N, mask_zero, out);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}
