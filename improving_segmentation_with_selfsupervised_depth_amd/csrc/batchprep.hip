// Device side of the data loader (loader/sequence_segmentation_loader.py:203-342 plus collation): decoded uint8 frames in,
// the training `inputs` tensors out.  Everything is integer arithmetic or one correctly rounded division, so every output is
// bit-identical to what PIL + ToTensor produce on the host:
//   crop_rgb_kernel   get_color's flip, random_crop's crop, ToTensor            (:145-150, :259-267, :319)
//   pyramid_kernel    transforms.Resize(..., Image.ANTIALIAS) by exactly 2, chained level to level, + ToTensor  (:308-309, :319)
//   labels_kernel     crop + flip + encode_segmap (a 256-entry table) + the one-hot planes              (:227-248, :324-327)
//   labels_rgb_kernel the same for colour-coded label maps: Mapillary's encode_segmap, a colour table in LDS
//                     (mapillary_vistas_loader.py:58-66)
//   plane_kernel      crop + flip + ToTensor of the one-channel pseudo_depth image                      (:272-273, :329-330)
//   jitter_*_kernel   the PIL ColorJitter of color_aug (brightness / contrast / saturation / hue in a drawn order) + ToTensor
//                     (:297-301, :318-322); Pillow's 8-bit arithmetic restated, fp32 and fp64 exactly where Pillow uses them
// The 8-bit level images stay planar ([planes][H][W], one plane per sample and channel): the pyramid reads them with 16-byte
// loads and ToTensor's CHW float planes are written next to them from the same registers.
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)
typedef unsigned bp_u32x4 __attribute__((ext_vector_type(4)));

// crop offsets are device data: an offset outside [0, frame - crop] is pulled back inside, never followed out of the tensor
__device__ __forceinline__ int crop_origin(const int* crop_xy, int i, int room) {
  const int v = crop_xy ? crop_xy[i] : 0;
  return v < 0 ? 0 : (v > room ? room : v);
}
// ToTensor: uint8 / 255 in fp32, correctly rounded (Markstein's two-fma division by a constant, as div_by<C> of loss.hip; the
// 256 possible inputs are compared with the IEEE quotient in tests/test_device_batch_emu.py and on the GPU)
__device__ __forceinline__ float unit_from_u8(unsigned v) {
  constexpr float rc = 1.f / 255.f;
  const float x = (float)v, q = x * rc;
  return __builtin_fmaf(__builtin_fmaf(-255.f, q, x), rc, q);
}

// ---------------------------------------------------------------------------------------------------------------------
// crop + flip + ToTensor of an HWC frame.  One wave owns CROP_SEG output pixels of one row: their 3 * CROP_SEG source bytes
// are contiguous whether or not the sample is flipped (a flip only reverses the pixel order), so the wave fetches them as
// 16-byte aligned chunks into LDS (whatever the crop offset makes of the alignment) and every lane then turns four
// neighbouring pixels into one 16-byte store per float plane and one 4-byte store per uint8 plane.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CROP_SEG = 256;                       // pixels per wave
constexpr int CROP_LDS = 3 * CROP_SEG + 32;         // + the chunk alignment slack on both sides

__global__ __launch_bounds__(256) void crop_rgb_kernel(const uint8_t* frames, long frame_bytes, int H, int W, const int* crop_xy,
                                                       const uint8_t* flip, int ch, int cw, uint8_t* u8, float* f32, int vec) {
  SEGSDE_SMEM;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t* sm = segsde_smem + wv * CROP_LDS;
  const int b = blockIdx.z, y = blockIdx.y * 4 + wv, x0 = blockIdx.x * CROP_SEG;
  const int x1 = crop_origin(crop_xy, 2 * b, W - cw), y1 = crop_origin(crop_xy, 2 * b + 1, H - ch);
  const bool fl = flip && flip[b];
  const int n = cw - x0 < CROP_SEG ? cw - x0 : CROP_SEG;
  const bool live = y < ch;
  int skew = 0;
  if (live) {
    // flip, then crop: output x reads source column W - 1 - (x1 + x) of a flipped sample
    const int sx = fl ? W - (x1 + x0 + n) : x1 + x0;
    const long first = (((long)b * H + y1 + y) * W + sx) * 3, last = first + 3L * n;      // byte range inside `frames`
    skew = (int)(reinterpret_cast<uintptr_t>(frames + first) & 15);
    const int chunks = (skew + 3 * n + 15) >> 4;                                           // <= 49
    if (lane < chunks) {
      const long at = first - skew + 16L * lane;
      bp_u32x4 v;
      if (at >= 0 && at + 16 <= frame_bytes) {
        v = *reinterpret_cast<const bp_u32x4*>(frames + at);
      } else {                                    // the chunk sticks out of the tensor: only the bytes of this segment are read
        unsigned w[4] = {0u, 0u, 0u, 0u};
        for (int i = 0; i < 16; ++i)
          if (at + i >= first && at + i < last) w[i >> 2] |= (unsigned)frames[at + i] << (8 * (i & 3));
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
      }
      *reinterpret_cast<bp_u32x4*>(sm + 16 * lane) = v;
    }
  }
  __syncthreads();
  if (!live || 4 * lane >= n) return;
  const uint8_t* px = sm + skew;
  const long plane = (long)ch * cw, o = ((long)b * 3 * ch + y) * cw + x0 + 4 * lane;
  if (vec) {                                      // cw % 4 == 0: whole groups of four
    for (int c = 0; c < 3; ++c) {
      unsigned q[4];
      for (int k = 0; k < 4; ++k) {
        const int i = 4 * lane + k;
        q[k] = px[3 * (fl ? n - 1 - i : i) + c];
      }
      *reinterpret_cast<unsigned*>(u8 + o + c * plane) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
      *reinterpret_cast<float4*>(f32 + o + c * plane) =
          make_float4(unit_from_u8(q[0]), unit_from_u8(q[1]), unit_from_u8(q[2]), unit_from_u8(q[3]));
    }
  } else {
    for (int k = 0; k < 4 && 4 * lane + k < n; ++k) {
      const int i = 4 * lane + k;
      for (int c = 0; c < 3; ++c) {
        const unsigned q = px[3 * (fl ? n - 1 - i : i) + c];
        u8[o + k + c * plane] = (uint8_t)q;
        f32[o + k + c * plane] = unit_from_u8(q);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// One pyramid level: Pillow's 8-bit resampler (Resample.c) for the Lanczos filter at an exact reduction by 2.
//   pass 1 (horizontal), pass 2 (vertical), a uint8 image in between; per output  clip8((2^21 + sum_j k[j] * pix[j]) >> 22)
//   with k[j] = (int)(w[j] * 2^22 +- 0.5), w = the normalised float64 window sinc(x) sinc(x / 3) of support 6.
// Output xx reads the 12 source pixels 2 xx - 5 .. 2 xx + 6; windows cut by a border are renormalised by Pillow, so the first
// three and the last three outputs of an axis have coefficient sets of their own.  The table comes from the host (float64,
// Pillow's formula): per axis 7 rows x 12 taps, taps outside the image zero; output xx of an axis of n outputs uses row
//   xx                     for xx < 3          (left border)
//   R - (n - xx)           for xx >= n - 3     (right border; R = min(n, 7) rows are in use)
//   3                      otherwise           (interior: every window whole, one set for all)
// A block makes PYR_W x PYR_H outputs of one plane: source tile + halo into LDS (16-byte loads when the rows allow it),
// horizontal pass LDS -> LDS (rounded and clipped to uint8, as Pillow's intermediate image is), vertical pass LDS -> global.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PYR_W = 64, PYR_H = 16;                 // outputs per block (tests/device_batch_cases.py: case B spans several)
constexpr int PYR_TAPS = 12, PYR_ROWS = 7;
constexpr int PYR_SRC_ROWS = 2 * PYR_H + 10;          // 5 rows of halo above, 5 below (the 12-tap window of an even reduction)
constexpr int PYR_SRC_PITCH = 2 * PYR_W + 32;         // tile column 0 = source column 2 * tx0 - 16: chunks stay 16-byte aligned
constexpr int PYR_COEF_BYTES = 2 * PYR_ROWS * PYR_TAPS * 4;
constexpr int PYR_SRC_BYTES = PYR_SRC_ROWS * PYR_SRC_PITCH;
constexpr int PYR_MID_BYTES = PYR_SRC_ROWS * PYR_W;
constexpr int PYR_LDS = PYR_COEF_BYTES + PYR_SRC_BYTES + PYR_MID_BYTES;
static_assert(PYR_COEF_BYTES % 16 == 0 && PYR_SRC_BYTES % 16 == 0, "LDS regions stay 16-byte aligned");
static_assert(PYR_W * PYR_H == 4 * 256, "vertical pass: four outputs per thread");

__device__ __forceinline__ int pyr_row(int xx, int n) {
  const int R = n < PYR_ROWS ? n : PYR_ROWS;
  return xx < 3 ? xx : (xx >= n - 3 ? R - (n - xx) : 3);
}
__device__ __forceinline__ unsigned pyr_clip8(int acc) {
  const int v = acc >> 22;                            // arithmetic shift: Pillow indexes its clip table with ss >> PRECISION_BITS
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(256) void pyramid_kernel(const uint8_t* src, int Hs, int Ws, const int* coef, int Hd, int Wd,
                                                      uint8_t* u8, float* f32, int vec_in, int vec_out) {
  SEGSDE_SMEM;
  int* ck = reinterpret_cast<int*>(segsde_smem);                        // [2][7][12]: the y rows, then the x rows
  uint8_t* ssrc = segsde_smem + PYR_COEF_BYTES;                          // [PYR_SRC_ROWS][PYR_SRC_PITCH]
  uint8_t* smid = ssrc + PYR_SRC_BYTES;                                  // [PYR_SRC_ROWS][PYR_W]
  const int t = threadIdx.x;
  const int tx0 = blockIdx.x * PYR_W, ty0 = blockIdx.y * PYR_H;
  const uint8_t* sp = src + (long)blockIdx.z * Hs * Ws;
  if (t < 2 * PYR_ROWS * PYR_TAPS) ck[t] = coef[t];
  const int sy0 = 2 * ty0 - 5, sx0 = 2 * tx0 - 16;
  if (vec_in) {                                       // Ws % 16 == 0, aligned base: a chunk is inside the row or outside it
    constexpr int CPR = PYR_SRC_PITCH / 16;
    for (int e = t; e < PYR_SRC_ROWS * CPR; e += 256) {
      const int r = e / CPR, j = e - r * CPR, sy = sy0 + r, c0 = sx0 + 16 * j;
      bp_u32x4 v = {0u, 0u, 0u, 0u};
      if (sy >= 0 && sy < Hs && c0 >= 0 && c0 + 16 <= Ws) v = *reinterpret_cast<const bp_u32x4*>(sp + (long)sy * Ws + c0);
      *reinterpret_cast<bp_u32x4*>(ssrc + r * PYR_SRC_PITCH + 16 * j) = v;
    }
  } else {
    for (int e = t; e < PYR_SRC_BYTES; e += 256) {
      const int r = e / PYR_SRC_PITCH, c = e - r * PYR_SRC_PITCH, sy = sy0 + r, sx = sx0 + c;
      ssrc[e] = (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) ? sp[(long)sy * Ws + sx] : (uint8_t)0;
    }
  }
  __syncthreads();
  // horizontal pass: an item is four neighbouring outputs of one tile row; their windows span 18 source bytes, fetched as
  // the six dwords from tile column 8 g + 8 (output 4 g + k, tap j = tile column 2 (4 g + k) + 11 + j = byte 3 + 2 k + j)
  const int* kx = ck + PYR_ROWS * PYR_TAPS;
  for (int e = t; e < PYR_SRC_ROWS * (PYR_W / 4); e += 256) {
    const int r = e / (PYR_W / 4), g = e - r * (PYR_W / 4);
    const unsigned* row = reinterpret_cast<const unsigned*>(ssrc + r * PYR_SRC_PITCH + 8 * g + 8);
    unsigned w[6];
    for (int i = 0; i < 6; ++i) w[i] = row[i];
    unsigned packed = 0u;
    for (int k = 0; k < 4; ++k) {
      const int xx = tx0 + 4 * g + k;
      if (xx >= Wd) break;
      const int* kr = kx + pyr_row(xx, Wd) * PYR_TAPS;
      int acc = 1 << 21;
      for (int j = 0; j < PYR_TAPS; ++j) {
        const int i = 3 + 2 * k + j;
        acc += kr[j] * (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
      }
      packed |= pyr_clip8(acc) << (8 * k);
    }
    *reinterpret_cast<unsigned*>(smid + r * PYR_W + 4 * g) = packed;
  }
  __syncthreads();
  // vertical pass: thread = four neighbouring outputs of one row; output row yl reads the rows 2 yl .. 2 yl + 11 of the tile
  const int g = t & 15, yl = t >> 4, yy = ty0 + yl, xx0 = tx0 + 4 * g;
  if (yy >= Hd || xx0 >= Wd) return;
  const int* kr = ck + pyr_row(yy, Hd) * PYR_TAPS;
  int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
  for (int j = 0; j < PYR_TAPS; ++j) {
    const unsigned w = *reinterpret_cast<const unsigned*>(smid + (2 * yl + j) * PYR_W + 4 * g);
    const int kj = kr[j];
    for (int k = 0; k < 4; ++k) acc[k] += kj * (int)((w >> (8 * k)) & 255u);
  }
  unsigned q[4];
  for (int k = 0; k < 4; ++k) q[k] = pyr_clip8(acc[k]);
  const long o = ((long)blockIdx.z * Hd + yy) * Wd + xx0;
  if (vec_out) {                                      // Wd % 4 == 0, aligned bases
    *reinterpret_cast<unsigned*>(u8 + o) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    *reinterpret_cast<float4*>(f32 + o) = make_float4(unit_from_u8(q[0]), unit_from_u8(q[1]), unit_from_u8(q[2]), unit_from_u8(q[3]));
  } else {
    for (int k = 0; k < 4 && xx0 + k < Wd; ++k) { u8[o + k] = (uint8_t)q[k]; f32[o + k] = unit_from_u8(q[k]); }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// one-channel maps: a thread per output pixel (the int64 / fp32 outputs are 8x / 4x the bytes of the uint8 input)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long crop_src(int b, int y, int x, int H, int W, const int* crop_xy, const uint8_t* flip, int ch, int cw) {
  const int x1 = crop_origin(crop_xy, 2 * b, W - cw), y1 = crop_origin(crop_xy, 2 * b + 1, H - ch);
  const int sx = (flip && flip[b]) ? W - 1 - (x1 + x) : x1 + x;
  return ((long)b * H + y1 + y) * W + sx;
}
__global__ __launch_bounds__(256) void labels_kernel(const uint8_t* lbl, int B, int H, int W, const int* crop_xy, const uint8_t* flip,
                                                     int ch, int cw, const int64_t* lut, const uint8_t* is_labeled,
                                                     int64_t ignore_index, int n_classes, int64_t* out, int64_t* onehot) {
  const long HW = (long)ch * cw, total = (long)B * HW;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int b = (int)(e / HW);
    const long p = e - b * HW;
    const int y = (int)(p / cw), x = (int)(p - (long)y * cw);
    const bool labeled = !is_labeled || is_labeled[b];
    const int64_t v = labeled ? lut[lbl[crop_src(b, y, x, H, W, crop_xy, flip, ch, cw)]] : ignore_index;
    out[e] = v;
    if (onehot) {                                     // ignore pixels and unlabeled samples: every plane zero
      int64_t* oh = onehot + (long)b * n_classes * HW + p;
      for (int c = 0; c < n_classes; ++c) oh[c * HW] = (labeled && v == c) ? 1 : 0;
    }
  }
}
// colour-coded label maps (mapillary_vistas_loader.py:58-66): the id of a pixel is the LAST colour of the table that equals its
// RGB triple, 0 when none does; the id `ignore_id` (Mapillary's "unlabeled", 65) becomes ignore_index.  The table sits in LDS as
// packed r | g << 8 | b << 16 words; every lane walks it in step, so the reads are broadcasts.
__global__ __launch_bounds__(256) void labels_rgb_kernel(const uint8_t* lbl, int B, int H, int W, const int* crop_xy, const uint8_t* flip,
                                                         int ch, int cw, const int* colors, int n_colors, int ignore_id,
                                                         const uint8_t* is_labeled, int64_t ignore_index, int n_classes, int64_t* out,
                                                         int64_t* onehot) {
  SEGSDE_SMEM;
  int* sc = reinterpret_cast<int*>(segsde_smem);
  for (int i = threadIdx.x; i < n_colors; i += 256) sc[i] = colors[i] & 0xffffff;
  __syncthreads();
  const long HW = (long)ch * cw, total = (long)B * HW;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int b = (int)(e / HW);
    const long p = e - b * HW;
    const int y = (int)(p / cw), x = (int)(p - (long)y * cw);
    const bool labeled = !is_labeled || is_labeled[b];
    int64_t v = ignore_index;
    if (labeled) {
      const uint8_t* px = lbl + 3 * crop_src(b, y, x, H, W, crop_xy, flip, ch, cw);
      const int rgb = (int)px[0] | ((int)px[1] << 8) | ((int)px[2] << 16);
      int id = 0;
      for (int l = 0; l < n_colors; ++l) id = sc[l] == rgb ? l : id;
      v = id == ignore_id ? ignore_index : (int64_t)id;
    }
    out[e] = v;
    if (onehot) {
      int64_t* oh = onehot + (long)b * n_classes * HW + p;
      for (int c = 0; c < n_classes; ++c) oh[c * HW] = (labeled && v == c) ? 1 : 0;
    }
  }
}
__global__ __launch_bounds__(256) void plane_kernel(const uint8_t* src, int B, int H, int W, const int* crop_xy, const uint8_t* flip,
                                                    int ch, int cw, float* out) {
  const long HW = (long)ch * cw, total = (long)B * HW;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int b = (int)(e / HW);
    const long p = e - b * HW;
    const int y = (int)(p / cw), x = (int)(p - (long)y * cw);
    out[e] = unit_from_u8(src[crop_src(b, y, x, H, W, crop_xy, flip, ch, cw)]);
  }
}
// ---------------------------------------------------------------------------------------------------------------------
// color_aug: torchvision's PIL ColorJitter on the level-0 crop.  Four operations, applied in the sample's drawn order with an
// 8-bit image between every two of them; every pixel is independent except for contrast, whose degenerate image is the mean L
// of the image AS IT STANDS when contrast's turn comes.  So: jitter_stats_kernel runs the operations in front of contrast and
// sums L (integer atomics: the sum does not depend on the order of the additions), jitter_apply_kernel runs them again from
// the source bytes, forms the mean and goes on.  No intermediate image is stored.
//   ImageEnhance.* end in Image.blend(degenerate, image, alpha): fp32  t = d + alpha * (x - d), truncated; clipped to 0..255
//   only when alpha is outside [0, 1] (inside, t cannot leave the range).  Degenerates: 0 (brightness), the image's mean L
//   (contrast), the pixel's own L (saturation).  L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16.
//   hue: RGB -> HSV (8 bit each), H += shift mod 256, HSV -> RGB; Pillow computes these in float with some subexpressions in
//   double, and the results depend on which -- the types below are Pillow's.  No product-sum here may become an fma.
// The operation id only selects a switch case and nothing is indexed with it, so a corrupt `order` table cannot lead a read
// out of range (the Python layer rejects a row that is no permutation before it is uploaded).
// ---------------------------------------------------------------------------------------------------------------------
enum { JIT_BRIGHTNESS = 0, JIT_CONTRAST = 1, JIT_SATURATION = 2, JIT_HUE = 3 };
constexpr int JIT_PX = 4;                             // pixels per thread: one dword per uint8 plane, one float4 per float plane

struct jit_rgb { int r, g, b; };

__device__ __forceinline__ int jit_luma(const jit_rgb& p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 0x8000) >> 16; }
__device__ __forceinline__ int jit_blend(int d, int x, float alpha, bool clip) {
#pragma clang fp contract(off)
  const float t = (float)d + alpha * (float)(x - d);
  if (clip) return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
  return (int)t;
}
__device__ __forceinline__ jit_rgb jit_blend3(int dr, int dg, int db, const jit_rgb& p, float alpha) {
  const bool clip = !(alpha >= 0.f && alpha <= 1.f);
  return jit_rgb{jit_blend(dr, p.r, alpha, clip), jit_blend(dg, p.g, alpha, clip), jit_blend(db, p.b, alpha, clip)};
}
__device__ __forceinline__ int jit_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// round half away from zero of a non-negative double, then the clip to 0..255
__device__ __forceinline__ int jit_round8(double x) {
  const double fl = floor(x);
  return jit_clip8((int)fl + ((x - fl) >= 0.5 ? 1 : 0));
}
__device__ __forceinline__ jit_rgb jit_hue(const jit_rgb& p, int shift) {
#pragma clang fp contract(off)
  const int mx = p.r > p.g ? (p.r > p.b ? p.r : p.b) : (p.g > p.b ? p.g : p.b);
  const int mn = p.r < p.g ? (p.r < p.b ? p.r : p.b) : (p.g < p.b ? p.g : p.b);
  int H = 0, S = 0;
  const int V = mx;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - p.r) / cr, gc = (float)(mx - p.g) / cr, bc = (float)(mx - p.b) / cr;
    float h;
    if (p.r == mx) h = bc - gc;
    else if (p.g == mx) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double u = (double)h / 6.0 + 1.0;           // in (5/6, 11/6): fmod(u, 1.0) is u or the exact difference u - 1
    const float hf = (float)(u >= 1.0 ? u - 1.0 : u);
    H = jit_clip8((int)((double)hf * 255.0));
    S = jit_clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) return jit_rgb{V, V, V};
  const double x = (double)H * 6.0 / 255.0;
  const double fi = floor(x);
  const float f = (float)(x - fi);
  const float fs = (float)((double)S / 255.0);
  const double dv = (double)V, dfs = (double)fs, df = (double)f;
  const int pp = jit_round8(dv * (1.0 - dfs));
  const int q = jit_round8(dv * (1.0 - dfs * df));
  const int t = jit_round8(dv * (1.0 - dfs * (1.0 - df)));
  switch ((int)fi % 6) {
    case 0: return jit_rgb{V, t, pp};
    case 1: return jit_rgb{q, V, pp};
    case 2: return jit_rgb{pp, V, t};
    case 3: return jit_rgb{pp, q, V};
    case 4: return jit_rgb{t, pp, V};
    default: return jit_rgb{V, pp, q};
  }
}
// the sample's tables, read once per thread (wave-uniform: scalar loads)
struct jit_params { float alpha[3]; int shift; unsigned order, ops; };      // order: four 2-bit operation ids, first in the low bits
__device__ __forceinline__ jit_params jit_load(int b, const float* alpha, const int* hue_shift, const uint8_t* order, int ops) {
  jit_params P;
  P.ops = (unsigned)ops;
  for (int i = 0; i < 3; ++i) P.alpha[i] = alpha[3 * b + i];
  P.shift = hue_shift[b] & 255;
  P.order = 0u;
  for (int i = 0; i < 4; ++i) P.order |= (unsigned)(order[4 * b + i] & 3) << (2 * i);
  return P;
}
// the operations at positions [from, 4) of the order that the mask `ops` (bit = operation id) enables, stopping in front of
// contrast when `mean` < 0; returns the position it stopped at (4: all done)
__device__ __forceinline__ int jit_run(jit_rgb& p, const jit_params& P, int from, int mean) {
  for (int i = from; i < 4; ++i) {
    const unsigned op = (P.order >> (2 * i)) & 3u;
    if (!((P.ops >> op) & 1u)) continue;
    switch (op) {
      case JIT_BRIGHTNESS: p = jit_blend3(0, 0, 0, p, P.alpha[0]); break;
      case JIT_CONTRAST:
        if (mean < 0) return i;
        p = jit_blend3(mean, mean, mean, p, P.alpha[1]);
        break;
      case JIT_SATURATION: { const int l = jit_luma(p); p = jit_blend3(l, l, l, p, P.alpha[2]); break; }
      default: p = jit_hue(p, P.shift); break;
    }
  }
  return 4;
}
__device__ __forceinline__ void jit_fetch(const uint8_t* img, long hw, long at, int vec, unsigned q[3][JIT_PX]) {
  for (int c = 0; c < 3; ++c) {
    if (vec) {
      const unsigned w = *reinterpret_cast<const unsigned*>(img + c * hw + at);
      for (int k = 0; k < JIT_PX; ++k) q[c][k] = (w >> (8 * k)) & 255u;
    } else {
      for (int k = 0; k < JIT_PX; ++k) q[c][k] = at + k < hw ? img[c * hw + at + k] : 0u;
    }
  }
}

// grid: (chunks of 256 * JIT_PX pixels, images); image i belongs to sample i % B.  sums[i] += the L of every pixel after the
// operations in front of contrast.
__global__ __launch_bounds__(256) void jitter_stats_kernel(const uint8_t* u8, int B, long hw, const uint8_t* apply, const float* alpha,
                                                           const int* hue_shift, const uint8_t* order, int ops, unsigned* sums, int vec) {
  const int img = blockIdx.y, b = img % B;
  if (!apply[b]) return;                              // the whole block: no lane is left waiting in the reduction below
  const jit_params P = jit_load(b, alpha, hue_shift, order, ops);
  const long at = ((long)blockIdx.x * 256 + threadIdx.x) * JIT_PX;
  int sum = 0;
  if (at < hw) {
    unsigned q[3][JIT_PX];
    jit_fetch(u8 + (long)img * 3 * hw, hw, at, vec, q);
    for (int k = 0; k < JIT_PX; ++k) {
      if (at + k >= hw) break;
      jit_rgb p{(int)q[0][k], (int)q[1][k], (int)q[2][k]};
      jit_run(p, P, 0, -1);
      sum += jit_luma(p);
    }
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);           // <= 64 * 4 * 255
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(sums + img, (unsigned)sum);
}

__global__ __launch_bounds__(256) void jitter_apply_kernel(const uint8_t* u8, int B, long hw, const uint8_t* apply, const float* alpha,
                                                           const int* hue_shift, const uint8_t* order, int ops, const unsigned* sums,
                                                           float* f32, int vec) {
  const int img = blockIdx.y, b = img % B;
  const long at = ((long)blockIdx.x * 256 + threadIdx.x) * JIT_PX;
  if (at >= hw) return;
  unsigned q[3][JIT_PX];
  jit_fetch(u8 + (long)img * 3 * hw, hw, at, vec, q);
  if (apply[b]) {
    const jit_params P = jit_load(b, alpha, hue_shift, order, ops);
    // ImageStat mean + 0.5, truncated:  (2 sum + n) / (2 n)  in integers
    const int mean = (int)((2ull * sums[img] + (unsigned long long)hw) / (2ull * (unsigned long long)hw));
    for (int k = 0; k < JIT_PX; ++k) {
      if (at + k >= hw) break;
      jit_rgb p{(int)q[0][k], (int)q[1][k], (int)q[2][k]};
      const int stop = jit_run(p, P, 0, -1);
      if (stop < 4) jit_run(p, P, stop, mean);
      q[0][k] = (unsigned)p.r; q[1][k] = (unsigned)p.g; q[2][k] = (unsigned)p.b;
    }
  }
  float* out = f32 + (long)img * 3 * hw + at;
  for (int c = 0; c < 3; ++c) {
    if (vec) {
      *reinterpret_cast<float4*>(out + c * hw) =
          make_float4(unit_from_u8(q[c][0]), unit_from_u8(q[c][1]), unit_from_u8(q[c][2]), unit_from_u8(q[c][3]));
    } else {
      for (int k = 0; k < JIT_PX && at + k < hw; ++k) out[c * hw + k] = unit_from_u8(q[c][k]);
    }
  }
}

inline int flat_blocks(long n) { long nb = (n + 255) / 256; return (int)(nb < 1 ? 1 : (nb > 8192 ? 8192 : nb)); }
inline bool crop_shape_ok(int B, int H, int W, int ch, int cw) {
  return B > 0 && H > 0 && W > 0 && ch > 0 && cw > 0 && ch <= H && cw <= W && B <= 65535;
}
inline bool aligned16(const void* a, const void* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}
}  // namespace

extern "C" int segsde_batchprep_crop(const uint8_t* frames, int B, int H, int W, const int32_t* crop_xy, const uint8_t* flip,
                                     int ch, int cw, uint8_t* u8_out, float* f32_out, void* stream) {
  if (!frames || !u8_out || !f32_out) return SEGSDE_ERR_NULL;
  if (!crop_shape_ok(B, H, W, ch, cw)) return SEGSDE_ERR_SHAPE;
  if ((!crop_xy && (ch != H || cw != W)) || (long)segsde_cdiv(ch, 4) > 65535) return SEGSDE_ERR_SHAPE;
  const int vec = (cw & 3) == 0 && aligned16(f32_out, nullptr) && (reinterpret_cast<uintptr_t>(u8_out) & 3) == 0;
  hipLaunchKernelGGL(crop_rgb_kernel, dim3(segsde_cdiv(cw, CROP_SEG), segsde_cdiv(ch, 4), B), dim3(256), 4 * CROP_LDS, ST(stream),
                     frames, (long)B * H * W * 3, H, W, crop_xy, flip, ch, cw, u8_out, f32_out, vec);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_batchprep_pyramid_level(const uint8_t* src, int planes, int Hs, int Ws, const int32_t* coef, int Hd, int Wd,
                                              uint8_t* u8_out, float* f32_out, void* stream) {
  if (!src || !coef || !u8_out || !f32_out) return SEGSDE_ERR_NULL;
  if (planes <= 0 || planes > 65535 || Hd <= 0 || Wd <= 0 || Hs != 2 * Hd || Ws != 2 * Wd) return SEGSDE_ERR_SHAPE;
  if (segsde_cdiv(Hd, PYR_H) > 65535) return SEGSDE_ERR_SHAPE;
  const int vec_in = (Ws & 15) == 0 && aligned16(src, nullptr);
  const int vec_out = (Wd & 3) == 0 && aligned16(f32_out, nullptr) && (reinterpret_cast<uintptr_t>(u8_out) & 3) == 0;
  hipLaunchKernelGGL(pyramid_kernel, dim3(segsde_cdiv(Wd, PYR_W), segsde_cdiv(Hd, PYR_H), planes), dim3(256), PYR_LDS, ST(stream), src,
                     Hs, Ws, coef, Hd, Wd, u8_out, f32_out, vec_in, vec_out);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_batchprep_labels(const uint8_t* lbl, int B, int H, int W, const int32_t* crop_xy, const uint8_t* flip, int ch,
                                       int cw, const int64_t* lut, const uint8_t* is_labeled, int64_t ignore_index, int n_classes,
                                       int64_t* lbl_out, int64_t* onehot_out, void* stream) {
  if (!lbl || !lut || !lbl_out) return SEGSDE_ERR_NULL;
  if (!crop_shape_ok(B, H, W, ch, cw) || (!crop_xy && (ch != H || cw != W)) || (onehot_out && n_classes <= 0)) return SEGSDE_ERR_SHAPE;
  hipLaunchKernelGGL(labels_kernel, dim3(flat_blocks((long)B * ch * cw)), dim3(256), 0, ST(stream), lbl, B, H, W, crop_xy, flip, ch, cw,
                     lut, is_labeled, ignore_index, n_classes, lbl_out, onehot_out);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_batchprep_labels_rgb(const uint8_t* lbl, int B, int H, int W, const int32_t* crop_xy, const uint8_t* flip, int ch,
                                           int cw, const int32_t* colors, int n_colors, int ignore_id, const uint8_t* is_labeled,
                                           int64_t ignore_index, int n_classes, int64_t* lbl_out, int64_t* onehot_out, void* stream) {
  if (!lbl || !colors || !lbl_out) return SEGSDE_ERR_NULL;
  if (!crop_shape_ok(B, H, W, ch, cw) || (!crop_xy && (ch != H || cw != W)) || (onehot_out && n_classes <= 0)) return SEGSDE_ERR_SHAPE;
  if (n_colors <= 0 || n_colors > SEGSDE_LABEL_COLORS_MAX) return SEGSDE_ERR_SHAPE;
  hipLaunchKernelGGL(labels_rgb_kernel, dim3(flat_blocks((long)B * ch * cw)), dim3(256), sizeof(int) * n_colors, ST(stream), lbl, B, H, W,
                     crop_xy, flip, ch, cw, colors, n_colors, ignore_id, is_labeled, ignore_index, n_classes, lbl_out, onehot_out);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_batchprep_plane(const uint8_t* src, int B, int H, int W, const int32_t* crop_xy, const uint8_t* flip, int ch,
                                      int cw, float* out, void* stream) {
  if (!src || !out) return SEGSDE_ERR_NULL;
  if (!crop_shape_ok(B, H, W, ch, cw) || (!crop_xy && (ch != H || cw != W))) return SEGSDE_ERR_SHAPE;
  hipLaunchKernelGGL(plane_kernel, dim3(flat_blocks((long)B * ch * cw)), dim3(256), 0, ST(stream), src, B, H, W, crop_xy, flip, ch, cw,
                     out);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_batchprep_color_jitter(const uint8_t* u8, int images, int B, int h, int w, const uint8_t* apply,
                                             const float* alpha, const int32_t* hue_shift, const uint8_t* order, int ops,
                                             uint32_t* sums, float* f32_out, void* stream) {
  if (!u8 || !apply || !alpha || !hue_shift || !order || !sums || !f32_out) return SEGSDE_ERR_NULL;
  if (images <= 0 || images > 65535 || B <= 0 || images % B != 0 || h <= 0 || w <= 0 || ops < 0 || ops > 15) return SEGSDE_ERR_SHAPE;
  const long hw = (long)h * w;
  if (hw > SEGSDE_COLOR_JITTER_MAX_PIXELS) return SEGSDE_ERR_SHAPE;      // 255 * hw must fit the uint32 sum
  const int vec = (hw & 3) == 0 && aligned16(f32_out, nullptr) && (reinterpret_cast<uintptr_t>(u8) & 3) == 0;
  const dim3 grid(segsde_cdiv(hw, 256L * JIT_PX), images);
  if (hipMemsetAsync(sums, 0, sizeof(uint32_t) * images, ST(stream)) != hipSuccess) return SEGSDE_ERR_NULL;
  hipLaunchKernelGGL(jitter_stats_kernel, grid, dim3(256), 0, ST(stream), u8, B, hw, apply, alpha, hue_shift, order, ops, sums, vec);
  SEGSDE_CHECK_LAUNCH();
  hipLaunchKernelGGL(jitter_apply_kernel, grid, dim3(256), 0, ST(stream), u8, B, hw, apply, alpha, hue_shift, order, ops, sums, f32_out, vec);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}
