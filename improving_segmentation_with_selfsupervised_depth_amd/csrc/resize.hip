// pil_loader's resize on the device (loader/loader_utils.py:23-43): decoded frames of any size -> the working size, in front
// of the stage of batchprep.hip.  Bit-identical to Pillow:
//   resample_rows_kernel / resample_cols_kernel   Image.resize(size, Image.ANTIALIAS) of an 8-bit RGB image: Resample.c for the
//                                                 Lanczos filter at any ratio, enlargement included
//   resize_nearest_kernel                         Image.resize(size, Image.NEAREST) of a label map (1 or 3 bytes per pixel)
// Resample.c: a horizontal pass, a uint8 image, a vertical pass; per output  clip8((2^21 + sum_j k[j] * pix[xmin + j]) >> 22)  in
// 32-bit integers, k[j] = (int)(w[j] * 2^22 +- 0.5) of the float64 Lanczos window of support 3 * max(in / out, 1), normalised
// after the cut at the image border.  A pass whose axis keeps its size is not run (Pillow skips it: no second rounding); the
// caller simply does not launch it.  The windows come from the host (float64, Pillow's formula; loader/device_batch.py): per
// axis and per distinct (in, out) pair  bounds int32 [out][2] = (xmin, count)  and  weights int32 [out][taps], taps = the
// table's pitch >= every count.  Samples of one launch may differ in source size: each has a descriptor (rs_desc) with its
// pointers, source size and tables; blockIdx.z walks the descriptors.
// Everything a descriptor or a table says is device data: window bounds are pulled inside the source and inside the LDS
// stage before they are followed, the tap count is cut to what the launch reserved.
#include "segsde_common.h"

namespace {
#define ST(s) static_cast<hipStream_t>(s)
typedef unsigned rs_u32x4 __attribute__((ext_vector_type(4)));

struct rs_desc {                      // mirror of the int64 [n][8] rows hipops uploads
  const uint8_t* src;
  uint8_t* dst;
  const int* bounds;                  // resample: [out][2] = (first source pixel, taps in use); nearest: source row of every output row
  const int* weights;                 // resample: [out][taps]; nearest: source column of every output column
  long in_h, in_w;                    // source rows / pixels per row (the column pass ignores in_w: its rows are `pitch` bytes)
  long taps;                          // pitch of `weights`
  long spare;
};
static_assert(sizeof(rs_desc) == 64, "eight 64-bit fields");

constexpr int RS_MAX_TAPS = SEGSDE_RESAMPLE_MAX_TAPS;
constexpr int RS_LDS_LIMIT = 64 * 1024;

__device__ __forceinline__ unsigned rs_clip8(int acc) {
  const int v = acc >> 22;            // arithmetic shift: Pillow indexes its clip table with ss >> PRECISION_BITS
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------------
// Horizontal pass over HWC rows: src [in_h][in_w][3] -> dst [in_h][Wd][3].  A block makes RSH_W output pixels of RSH_ROWS rows,
// RSH_R rows at a time: the windows and weights of its RSH_W outputs go to LDS once; per group of rows the source bytes all
// those windows cover (contiguous in a row: 3 * span bytes from pixel lo) are fetched as 16-byte aligned chunks into LDS,
// whatever the row's alignment is (the crop kernel's scheme: a chunk that sticks out of the sample is read byte by byte),
// every thread forms the three channels of one output from LDS, and the 192-byte output rows leave through LDS as 16-byte
// stores when the destination rows allow it.  Lane = output pixel: its weight row has an odd pitch in dwords whenever taps
// is odd (Pillow's ksize always is), so the weight reads spread over the banks.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int RSH_W = 64, RSH_R = 8, RSH_ROWS = 32;
constexpr int RSH_OUT_PITCH = 3 * RSH_W;
constexpr int RSH_HEAD_BYTES = (2 * RSH_W + 16) * 4;                    // bounds [64][2], the rows' skews [8] (+ padding)
constexpr int RSH_OUT_BYTES = RSH_R * RSH_OUT_PITCH;
static_assert(RSH_HEAD_BYTES % 16 == 0 && RSH_OUT_BYTES % 16 == 0 && RSH_OUT_PITCH % 16 == 0, "LDS regions stay 16-byte aligned");
static_assert(RSH_R == 8 && RSH_W == 64, "a wave stages two rows and computes two rows of 64 outputs");

__global__ __launch_bounds__(256) void resample_rows_kernel(const rs_desc* desc, int Wd, int kcap, int src_pitch) {
  SEGSDE_SMEM;
  int* sb = reinterpret_cast<int*>(segsde_smem);
  int* ssk = sb + 2 * RSH_W;
  uint8_t* sout = segsde_smem + RSH_HEAD_BYTES;                          // [RSH_R][RSH_OUT_PITCH]
  int* sw = reinterpret_cast<int*>(sout + RSH_OUT_BYTES);                // [RSH_W][ks]
  uint8_t* ssrc = reinterpret_cast<uint8_t*>(sw + RSH_W * kcap);         // [RSH_R][src_pitch]
  const rs_desc d = desc[blockIdx.z];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const int Hs = (int)d.in_h, Ws = (int)d.in_w;
  const int x0 = blockIdx.x * RSH_W, row0 = blockIdx.y * RSH_ROWS;
  if (row0 >= Hs || Ws <= 0) return;                                     // the whole block: samples differ in height
  const int ks = rs_clamp((int)d.taps, 1, kcap);
  const int nx = Wd - x0 < RSH_W ? Wd - x0 : RSH_W;
  if (t < nx) {
    const int xmin = rs_clamp(d.bounds[2 * (x0 + t)], 0, Ws);
    const int room = Ws - xmin < ks ? Ws - xmin : ks;
    sb[2 * t] = xmin;
    sb[2 * t + 1] = rs_clamp(d.bounds[2 * (x0 + t) + 1], 0, room);
  }
  for (int e = t; e < nx * ks; e += 256) sw[e] = d.weights[(long)x0 * ks + e];
  __syncthreads();
  // windows move right with the output: the first one starts the block's source range, the last one ends it
  const int lo = sb[0];
  const int span = rs_clamp(sb[2 * (nx - 1)] + sb[2 * (nx - 1) + 1] - lo, 0, (src_pitch - 32) / 3);
  int rel = 0, cnt = 0;
  if (lane < nx) {
    rel = rs_clamp(sb[2 * lane] - lo, 0, span);
    cnt = sb[2 * lane + 1] < span - rel ? sb[2 * lane + 1] : span - rel;
  }
  const int* kr = sw + lane * ks;
  const int rend = row0 + RSH_ROWS < Hs ? row0 + RSH_ROWS : Hs;
  const long total = (long)Hs * Ws * 3;
  const int row_bytes = 3 * Wd, nbytes = 3 * nx;
  const bool vec_out = ((reinterpret_cast<uintptr_t>(d.dst) | (uintptr_t)row_bytes) & 15) == 0;
  for (int r0 = row0; r0 < rend; r0 += RSH_R) {
    for (int rr = wv; rr < RSH_R; rr += 4) {
      const int y = r0 + rr;
      if (y >= rend) continue;
      const long first = ((long)y * Ws + lo) * 3, last = first + 3L * span;                 // byte range inside the sample
      const int skew = (int)(reinterpret_cast<uintptr_t>(d.src + first) & 15);
      if (lane == 0) ssk[rr] = skew;
      const int chunks = (skew + 3 * span + 15) >> 4;                                        // 16 * chunks <= src_pitch
      for (int c = lane; c < chunks; c += 64) {
        const long at = first - skew + 16L * c;
        rs_u32x4 v;
        if (at >= 0 && at + 16 <= total) {
          v = *reinterpret_cast<const rs_u32x4*>(d.src + at);
        } else {                                  // the chunk sticks out of the sample: only the bytes of this range are read
          unsigned w[4] = {0u, 0u, 0u, 0u};
          for (int i = 0; i < 16; ++i)
            if (at + i >= first && at + i < last) w[i >> 2] |= (unsigned)d.src[at + i] << (8 * (i & 3));
          v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        *reinterpret_cast<rs_u32x4*>(ssrc + rr * src_pitch + 16 * c) = v;
      }
    }
    __syncthreads();
    for (int rr = wv; rr < RSH_R; rr += 4) {
      if (r0 + rr >= rend || lane >= nx) continue;
      // a pixel's three bytes start anywhere: they are cut out of the two aligned dwords that hold them, so every LDS read is
      // an aligned one (the second dword stays inside the row's stage: 3 * span + 32 bytes are reserved, skew <= 15)
      const unsigned* row32 = reinterpret_cast<const unsigned*>(ssrc + rr * src_pitch);
      int at = ssk[rr] + 3 * rel;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int j = 0; j < cnt; ++j, at += 3) {
        const unsigned long long two = ((unsigned long long)row32[(at >> 2) + 1] << 32) | row32[at >> 2];
        const unsigned p = (unsigned)(two >> (8 * (at & 3)));
        const int k = kr[j];
        a0 += k * (int)(p & 255u);
        a1 += k * (int)((p >> 8) & 255u);
        a2 += k * (int)((p >> 16) & 255u);
      }
      uint8_t* o = sout + rr * RSH_OUT_PITCH + 3 * lane;
      o[0] = (uint8_t)rs_clip8(a0); o[1] = (uint8_t)rs_clip8(a1); o[2] = (uint8_t)rs_clip8(a2);
    }
    __syncthreads();
    uint8_t* out = d.dst + (long)r0 * row_bytes + 3L * x0;
    if (vec_out) {                                // rows start and end on 16-byte boundaries, and so does this block's part
      constexpr int CPR = RSH_OUT_PITCH / 16;
      for (int e = t; e < RSH_R * CPR; e += 256) {
        const int rr = e / CPR, c = e - rr * CPR;
        if (r0 + rr < rend && 16 * c < nbytes)
          *reinterpret_cast<rs_u32x4*>(out + (long)rr * row_bytes + 16 * c) = *reinterpret_cast<const rs_u32x4*>(sout + rr * RSH_OUT_PITCH + 16 * c);
      }
    } else {
      for (int e = t; e < RSH_OUT_BYTES; e += 256) {
        const int rr = e / RSH_OUT_PITCH, c = e - rr * RSH_OUT_PITCH;
        if (r0 + rr < rend && c < nbytes) out[(long)rr * row_bytes + c] = sout[e];
      }
    }
    // the next group's staging writes ssrc and ssk only; its barrier orders them after these reads of sout
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Vertical pass: src [in_h][pitch bytes] -> dst [Hd][pitch bytes].  The channels of a row are just neighbouring bytes, so the
// pass is a one-channel one over 3 * W byte columns.  A block makes RSV_H output rows of RSV_WB byte columns: the source rows
// its windows cover go to LDS (16-byte loads when the rows allow it), a thread then forms 16 neighbouring bytes of one output
// row -- one 16-byte LDS read per tap, one 16-byte store.  Coalesced along x in both directions.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int RSV_WB = 256, RSV_H = 16;
constexpr int RSV_HEAD_BYTES = 2 * RSV_H * 4;
static_assert(RSV_HEAD_BYTES % 16 == 0 && (RSV_WB / 16) * RSV_H == 256, "a thread per 16 bytes of an output row");

__global__ __launch_bounds__(256) void resample_cols_kernel(const rs_desc* desc, int pitch, int Hd, int kcap, int span_cap) {
  SEGSDE_SMEM;
  int* sb = reinterpret_cast<int*>(segsde_smem);                          // [RSV_H][2]
  int* sw = sb + 2 * RSV_H;                                               // [RSV_H][ks]
  uint8_t* ssrc = reinterpret_cast<uint8_t*>(sw + RSV_H * kcap);          // [span_cap][RSV_WB]
  const rs_desc d = desc[blockIdx.z];
  const int t = threadIdx.x, g = t & 15, yl = t >> 4;
  const int Hs = (int)d.in_h;
  if (Hs <= 0) return;
  const int y0 = blockIdx.y * RSV_H, c0 = blockIdx.x * RSV_WB;
  const int ks = rs_clamp((int)d.taps, 1, kcap);
  const int ny = Hd - y0 < RSV_H ? Hd - y0 : RSV_H, nb = pitch - c0 < RSV_WB ? pitch - c0 : RSV_WB;
  if (t < ny) {
    const int ymin = rs_clamp(d.bounds[2 * (y0 + t)], 0, Hs);
    const int room = Hs - ymin < ks ? Hs - ymin : ks;
    sb[2 * t] = ymin;
    sb[2 * t + 1] = rs_clamp(d.bounds[2 * (y0 + t) + 1], 0, room);
  }
  for (int e = t; e < ny * ks; e += 256) sw[e] = d.weights[(long)y0 * ks + e];
  __syncthreads();
  const int lo = sb[0];
  const int span = rs_clamp(sb[2 * (ny - 1)] + sb[2 * (ny - 1) + 1] - lo, 0, span_cap);
  const uint8_t* sp = d.src + (long)lo * pitch + c0;
  if (((reinterpret_cast<uintptr_t>(d.src) | (uintptr_t)pitch) & 15) == 0) {     // then nb is a multiple of 16: a chunk is inside the row or outside
    for (int e = t; e < span * (RSV_WB / 16); e += 256) {
      const int r = e >> 4, j = e & 15;
      rs_u32x4 v = {0u, 0u, 0u, 0u};
      if (16 * j < nb) v = *reinterpret_cast<const rs_u32x4*>(sp + (long)r * pitch + 16 * j);
      *reinterpret_cast<rs_u32x4*>(ssrc + r * RSV_WB + 16 * j) = v;
    }
  } else {
    for (int e = t; e < span * RSV_WB; e += 256) {
      const int r = e >> 8, c = e & 255;
      ssrc[e] = c < nb ? sp[(long)r * pitch + c] : (uint8_t)0;
    }
  }
  __syncthreads();
  if (yl >= ny || 16 * g >= nb) return;
  const int rel = rs_clamp(sb[2 * yl] - lo, 0, span);
  const int cnt = sb[2 * yl + 1] < span - rel ? sb[2 * yl + 1] : span - rel;
  const int* kr = sw + yl * ks;
  int acc[16];
  for (int i = 0; i < 16; ++i) acc[i] = 1 << 21;
  for (int j = 0; j < cnt; ++j) {
    const rs_u32x4 v = *reinterpret_cast<const rs_u32x4*>(ssrc + (rel + j) * RSV_WB + 16 * g);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    const int kj = kr[j];
    for (int q = 0; q < 4; ++q)
      for (int k = 0; k < 4; ++k) acc[4 * q + k] += kj * (int)((w[q] >> (8 * k)) & 255u);
  }
  // The clipped bytes are made opaque before they are packed: left to itself hipcc fuses  clip8(a >> 22) | clip8(b >> 22) << 8
  // into v_ashr_pk_u8_i32 and ORs the other two bytes onto its result as if the upper half of that register were zero; on the
  // MI355X the instruction leaves the upper half as it was, and bytes 2 of the later dwords came out ORed with stale ones.
  unsigned c8[16];
  for (int i = 0; i < 16; ++i) {
    c8[i] = rs_clip8(acc[i]);
    SEGSDE_OPAQUE(c8[i]);
  }
  unsigned q[4];
  for (int i = 0; i < 4; ++i) q[i] = c8[4 * i] | (c8[4 * i + 1] << 8) | (c8[4 * i + 2] << 16) | (c8[4 * i + 3] << 24);
  uint8_t* out = d.dst + (long)(y0 + yl) * pitch + c0 + 16 * g;
  if (((reinterpret_cast<uintptr_t>(d.dst) | (uintptr_t)pitch) & 15) == 0) {
    rs_u32x4 v;
    v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
    *reinterpret_cast<rs_u32x4*>(out) = v;
  } else {
    for (int i = 0; i < 16 && 16 * g + i < nb; ++i) out[i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Image.NEAREST: a gather through the per-axis index tables (Pillow accumulates a float64 step per output; the host restates
// that, Geometry.c ImagingScaleAffine).  grid: (chunks of pixels, samples)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resize_nearest_kernel(const rs_desc* desc, int Hd, int Wd, int C) {
  const rs_desc d = desc[blockIdx.y];
  const int Hs = (int)d.in_h, Ws = (int)d.in_w;
  if (Hs <= 0 || Ws <= 0) return;
  const long total = (long)Hd * Wd;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int y = (int)(e / Wd), x = (int)(e - (long)y * Wd);
    const int sy = rs_clamp(d.bounds[y], 0, Hs - 1), sx = rs_clamp(d.weights[x], 0, Ws - 1);
    const uint8_t* p = d.src + ((long)sy * Ws + sx) * C;
    for (int c = 0; c < C; ++c) d.dst[e * C + c] = p[c];
  }
}
}  // namespace

extern "C" int segsde_batchprep_resample_rows(const void* desc, int n, int max_rows, int Wd, int max_taps, int max_span,
                                              void* stream) {
  if (!desc) return SEGSDE_ERR_NULL;
  if (n <= 0 || n > 65535 || max_rows <= 0 || Wd <= 0 || max_taps <= 0 || max_span <= 0) return SEGSDE_ERR_SHAPE;
  if (max_taps > RS_MAX_TAPS) return SEGSDE_ERR_UNSUPPORTED;
  const long src_pitch = (3L * max_span + 32 + 15) & ~15L;
  const long lds = RSH_HEAD_BYTES + RSH_OUT_BYTES + 4L * RSH_W * max_taps + RSH_R * src_pitch;
  if (lds > RS_LDS_LIMIT) return SEGSDE_ERR_UNSUPPORTED;
  if (segsde_cdiv(max_rows, RSH_ROWS) > 65535) return SEGSDE_ERR_SHAPE;
  hipLaunchKernelGGL(resample_rows_kernel, dim3(segsde_cdiv(Wd, RSH_W), segsde_cdiv(max_rows, RSH_ROWS), n), dim3(256), (size_t)lds,
                     ST(stream), static_cast<const rs_desc*>(desc), Wd, max_taps, (int)src_pitch);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_batchprep_resample_cols(const void* desc, int n, int row_bytes, int Hd, int max_taps, int max_span,
                                              void* stream) {
  if (!desc) return SEGSDE_ERR_NULL;
  if (n <= 0 || n > 65535 || row_bytes <= 0 || Hd <= 0 || max_taps <= 0 || max_span <= 0) return SEGSDE_ERR_SHAPE;
  if (max_taps > RS_MAX_TAPS) return SEGSDE_ERR_UNSUPPORTED;
  const long lds = RSV_HEAD_BYTES + 4L * RSV_H * max_taps + (long)max_span * RSV_WB;
  if (lds > RS_LDS_LIMIT) return SEGSDE_ERR_UNSUPPORTED;
  if (segsde_cdiv(Hd, RSV_H) > 65535) return SEGSDE_ERR_SHAPE;
  hipLaunchKernelGGL(resample_cols_kernel, dim3(segsde_cdiv(row_bytes, RSV_WB), segsde_cdiv(Hd, RSV_H), n), dim3(256), (size_t)lds,
                     ST(stream), static_cast<const rs_desc*>(desc), row_bytes, Hd, max_taps, max_span);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}

extern "C" int segsde_batchprep_resize_nearest(const void* desc, int n, int Hd, int Wd, int channels, void* stream) {
  if (!desc) return SEGSDE_ERR_NULL;
  if (n <= 0 || n > 65535 || Hd <= 0 || Wd <= 0 || (channels != 1 && channels != 3)) return SEGSDE_ERR_SHAPE;
  long nb = ((long)Hd * Wd + 255) / 256;
  nb = nb > 4096 ? 4096 : nb;
  hipLaunchKernelGGL(resize_nearest_kernel, dim3((unsigned)nb, n), dim3(256), 0, ST(stream), static_cast<const rs_desc*>(desc), Hd, Wd,
                     channels);
  SEGSDE_CHECK_LAUNCH();
  return 0;
}
