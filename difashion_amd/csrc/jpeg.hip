// The JPEG save / open round trip: the pixels that `Image.fromarray(x).save(f, "JPEG", quality, subsampling)` followed
// by `Image.open(f).convert("RGB")` gives, without the byte stream.  Huffman coding is lossless, so the round trip is libjpeg's colour
// conversion, 2x2 chroma downsampling, the "islow" integer forward DCT, quantisation and the inverse of each -- the path PIL takes in
// both directions.  Every step is 32-bit integer arithmetic with fixed rounding (`>>` is arithmetic), so the result is the same in both
// storage builds and equal to PIL's bit for bit.  What the reference's evaluation scores is such a round trip of every generated item
// (inf4eval.py:787-790 writes "<i>.jpg", evaluate_gor.py:207-215 reads it back).
//
// Launch 1, jpeg_blocks_kernel: one workgroup owns a tile of TH x 64 pixels (4:2:0: TH = 16, four MCUs: 16 Y + 4 Cb + 4 Cr blocks;
// 4:4:4: TH = 8, eight MCUs: 8 Y + 8 Cb + 8 Cr blocks), 24 blocks of 8 x 8 either way, eight threads a block.  The RGB tile is staged
// in LDS with the image's last row / column replicated, converted (and downsampled) there into block-major samples; thread j of a block
// runs the 1-D pass of row j from registers, the block is transposed through LDS, the thread runs column j: forward DCT, quantise,
// dequantise, the column pass of the inverse DCT, all without leaving its registers; a second transpose, the row pass of the inverse,
// the range limit, and the decoded Y / Cb / Cr planes go to the workspace as whole 8-byte runs.  Launch 2, jpeg_pixels_kernel: per output
// pixel the "fancy" triangle upsampling of the chroma planes and YCbCr -> RGB, written HWC (four pixels a thread where w % 4 == 0).
// No atomics, nothing allocated, no per-thread array is indexed by a run-time value (zero scratch).
#include <cstdint>
#include <string>

#include "../../include/difashion_hip.h"
#include "dfh_common.h"

namespace {

constexpr int THREADS = 192;          // 24 blocks x 8 threads: three waves
constexpr int TILE_W = 64;            // pixels a tile is wide
constexpr int NBLK = 24;
constexpr int WS_STRIDE = 72;         // ints a block takes in the transpose buffer: 64 + 8, so the four blocks of a 32-lane group read
                                      // a column (stride 8 ints inside a block) from four different groups of eight of the 32 banks
constexpr int PIXELS_THREADS = 256;

// libjpeg jfdctint.c / jidctint.c: FIX(x) with CONST_BITS = 13, PASS1_BITS = 2
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
              F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

struct JpegArgs {
  const void* src; int src_kind;
  int batch, h, w, sub420;
  int tiles_x, tiles_y;
  int th;                              // rows a tile is high: 16 (4:2:0) / 8 (4:4:4)
  int ch, cw;                          // the chroma plane a decoder keeps: ceil(h / 2) x ceil(w / 2) (4:2:0), h x w (4:4:4)
  int yb_rows, yb_cols, cb_rows, cb_cols;     // real blocks of the luma plane, of one chroma plane
  int wy, hy, wc, hc;                  // the planes of the workspace, padded to whole tiles
  long plane_stride;                   // bytes of one image's three planes
  uint8_t* planes; int16_t* coef; uint8_t* dst;
  uint16_t q[2][64];                   // luminance / chrominance tables, natural order
};

DFH_DEVICE int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// difashion.postprocess(x, "pil") (image_processor.hip::quantise): x / 2 + 0.5, clamp to [0, 1], * 255, round half to even; NaN -> 0
DFH_DEVICE uint8_t quantise(float x) {
  float y = x * 0.5f + 0.5f;
  y = (y != y) ? 0.0f : fminf(fmaxf(y, 0.0f), 1.0f);
  return (uint8_t)(int)rintf(y * 255.0f);
}

DFH_DEVICE int rgb_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
DFH_DEVICE int rgb_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
DFH_DEVICE int rgb_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// Two horizontally adjacent pixels (xx even) of the staged RGB tile: six bytes on a 2-byte boundary, three 16-bit LDS reads
struct PixelPair {
  int r0, g0, b0, r1, g1, b1;
  DFH_DEVICE PixelPair(const uint8_t* stage, int yy, int xx) {
    const uint16_t* p = (const uint16_t*)(stage + (yy * TILE_W + xx) * 3);
    const int p0 = p[0], p1 = p[1], p2 = p[2];
    r0 = p0 & 255; g0 = p0 >> 8; b0 = p1 & 255; r1 = p1 >> 8; g1 = p2 & 255; b1 = p2 >> 8;
  }
};

// One 1-D pass of the forward "islow" DCT.  FIRST: the row pass (two extra bits kept, descale by 11); else the column pass (descale by
// 2 for outputs 0 and 4, by 15 for the others)
template <bool FIRST>
DFH_DEVICE void fdct_1d(int (&d)[8]) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int N = FIRST ? 11 : 15;
  d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * F_0_541;
  d[2] = descale(z1 + t13 * F_0_765, N);
  d[6] = descale(z1 - t12 * F_1_847, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F_1_175;
  const int u4 = t4 * F_0_298, u5 = t5 * F_2_053, u6 = t6 * F_3_072, u7 = t7 * F_1_501;
  z1 = -z1 * F_0_899; z2 = -z2 * F_2_562; z3 = -z3 * F_1_961 + z5; z4 = -z4 * F_0_390 + z5;
  d[7] = descale(u4 + z1 + z3, N);
  d[5] = descale(u5 + z2 + z4, N);
  d[3] = descale(u6 + z2 + z3, N);
  d[1] = descale(u7 + z1 + z4, N);
}

// One 1-D pass of the inverse "islow" DCT, descaled by N (11: the column pass, 18: the row pass)
template <int N>
DFH_DEVICE void idct_1d(int (&x)[8]) {
  int z1 = (x[2] + x[6]) * F_0_541;
  const int e2 = z1 - x[6] * F_1_847, e3 = z1 + x[2] * F_0_765;
  const int e0 = (x[0] + x[4]) * 8192, e1 = (x[0] - x[4]) * 8192;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * F_1_175;
  t0 *= F_0_298; t1 *= F_2_053; t2 *= F_3_072; t3 *= F_1_501;
  z1 = -z1 * F_0_899; z2 = -z2 * F_2_562; z3 = -z3 * F_1_961 + z5; z4 = -z4 * F_0_390 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  x[0] = descale(t10 + t3, N); x[7] = descale(t10 - t3, N);
  x[1] = descale(t11 + t2, N); x[6] = descale(t11 - t2, N);
  x[2] = descale(t12 + t1, N); x[5] = descale(t12 - t1, N);
  x[3] = descale(t13 + t0, N); x[4] = descale(t13 - t0, N);
}

// libjpeg's range-limit table as a function of v & 1023: it WRAPS beyond +-384 around the centre, it does not clamp
DFH_DEVICE int range_limit(int v) {
  const int i = v & 1023;
  return i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896));
}

// component (0 Y, 1 Cb, 2 Cr) and the block's row / column inside the tile's part of that component's plane
DFH_DEVICE void block_place(bool sub420, int blk, int& comp, int& by, int& bx) {
  if (sub420) {
    if (blk < 16) { comp = 0; by = blk >> 3; bx = blk & 7; }
    else { comp = 1 + ((blk - 16) >> 2); by = 0; bx = blk & 3; }
  } else {
    comp = blk >> 3; by = 0; bx = blk & 7;
  }
}

__global__ __launch_bounds__(THREADS) void jpeg_blocks_kernel(const JpegArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[16 * TILE_W * 3];     // the RGB tile, edge replicated
  __shared__ __attribute__((aligned(16))) uint8_t samp[NBLK * 64];            // [block][row][col]: samples in, decoded samples out
  __shared__ __attribute__((aligned(16))) int ws[NBLK * WS_STRIDE];           // [block][row][col] between the passes
  __shared__ __attribute__((aligned(16))) int16_t scoef[NBLK * 64];           // quantised coefficients, natural order
  __shared__ uint16_t sq[2 * 64];
  const int tid = threadIdx.x;
  const bool sub420 = a.sub420 != 0;
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x; bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const long b = bid / a.tiles_y;
  const int x0 = tx * TILE_W, y0 = ty * a.th;

  // ---- stage: the tile's pixels, rows and columns beyond the image read the last row / column
  if (tid < 128) sq[tid] = a.q[tid >> 6][tid & 63];
  const int npix = a.th * TILE_W;
  if (a.src_kind == DFH_IMGPROC_SRC_U8_HWC) {
    const uint8_t* src = (const uint8_t*)a.src + b * a.h * a.w * 3;
    if ((a.w & 3) == 0 && x0 + TILE_W <= a.w) {
      // a whole tile row is 192 bytes inside one image row, and with w % 4 == 0 (src is 16-byte aligned) it starts on a dword
      for (int i = tid; i < a.th * (TILE_W * 3 / 4); i += THREADS) {
        const int row = i / (TILE_W * 3 / 4), c = i - row * (TILE_W * 3 / 4);
        const int gy = min(y0 + row, a.h - 1);
        ((uint32_t*)stage)[i] = ((const uint32_t*)(src + ((long)gy * a.w + x0) * 3))[c];
      }
    } else {
      for (int i = tid; i < npix * 3; i += THREADS) {
        const int row = i / (TILE_W * 3), c = i - row * (TILE_W * 3), px = c / 3, k = c - px * 3;
        const int gy = min(y0 + row, a.h - 1), gx = min(x0 + px, a.w - 1);
        stage[i] = src[((long)gy * a.w + gx) * 3 + k];
      }
    }
  } else {
    const float* src = (const float*)a.src + b * 3 * a.h * a.w;
    for (int i = tid; i < npix * 3; i += THREADS) {
      const int k = i / npix, r = i - k * npix, row = r / TILE_W, px = r - row * TILE_W;
      const int gy = min(y0 + row, a.h - 1), gx = min(x0 + px, a.w - 1);
      stage[(row * TILE_W + px) * 3 + k] = quantise(src[((long)k * a.h + gy) * a.w + gx]);
    }
  }
  __syncthreads();

  // ---- colour conversion (and the 2 x 2 downsampling) into block-major samples
  if (sub420) {
    // one chroma sample = 2 x 2 pixels a step.  Rows: the image is replicated to an even row count only; below that it is the
    // DOWNSAMPLED last row that repeats, so a chroma row beyond the plane reads the plane's last row
    const int last_cy = a.ch - 1 - (y0 >> 1);
    for (int i = tid; i < 8 * 32; i += THREADS) {
      const int cy = i >> 5, cx = i & 31, cys = min(cy, last_cy);
      int sb = 0, sr = 0;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const int yy = 2 * cy + dy, xx = 2 * cx;
        PixelPair p(stage, yy, xx);
        *(uint16_t*)(samp + ((yy >> 3) * 8 + (xx >> 3)) * 64 + (yy & 7) * 8 + (xx & 7)) =
            (uint16_t)(rgb_y(p.r0, p.g0, p.b0) | (rgb_y(p.r1, p.g1, p.b1) << 8));
        if (cys != cy) p = PixelPair(stage, 2 * cys + dy, xx);     // only in the tiles of the image's last rows
        sb += rgb_cb(p.r0, p.g0, p.b0) + rgb_cb(p.r1, p.g1, p.b1);
        sr += rgb_cr(p.r0, p.g0, p.b0) + rgb_cr(p.r1, p.g1, p.b1);
      }
      const int bias = 1 + (cx & 1);                               // 1, 2, 1, 2 ... along the output columns
      const int o = (cx >> 3) * 64 + cy * 8 + (cx & 7);
      samp[16 * 64 + o] = (uint8_t)((sb + bias) >> 2);
      samp[20 * 64 + o] = (uint8_t)((sr + bias) >> 2);
    }
  } else {
    for (int i = tid; i < 8 * TILE_W; i += THREADS) {
      const int yy = i >> 6, xx = i & 63;
      const uint8_t* p = stage + i * 3;
      const int o = (xx >> 3) * 64 + yy * 8 + (xx & 7);
      samp[o] = (uint8_t)rgb_y(p[0], p[1], p[2]);
      samp[8 * 64 + o] = (uint8_t)rgb_cb(p[0], p[1], p[2]);
      samp[16 * 64 + o] = (uint8_t)rgb_cr(p[0], p[1], p[2]);
    }
  }
  __syncthreads();

  // ---- the block passes: thread j of block blk owns row j, then column j, then row j again
  const int blk = tid >> 3, j = tid & 7;
  int comp, by, bx;
  block_place(sub420, blk, comp, by, bx);
  int* w = ws + blk * WS_STRIDE;
  int v[8];
  {
    const uint2 s = *(const uint2*)(samp + blk * 64 + j * 8);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = (int)((s.x >> (8 * c)) & 255u) - 128;
      v[c + 4] = (int)((s.y >> (8 * c)) & 255u) - 128;
    }
  }
  fdct_1d<true>(v);
#pragma unroll
  for (int c = 0; c < 8; ++c) w[j * 8 + c] = v[c];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = w[r * 8 + j];
  fdct_1d<false>(v);
  const uint16_t* q = sq + (comp ? 64 : 0);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int qv = q[r * 8 + j], q8 = qv * 8, c = v[r];
    const int m = (int)((unsigned)((c < 0 ? -c : c) + (q8 >> 1)) / (unsigned)q8);      // the forward DCT leaves its output scaled by 8
    const int k = c < 0 ? -m : m;
    scoef[blk * 64 + r * 8 + j] = (int16_t)k;
    v[r] = k * qv;
  }
  idct_1d<11>(v);
#pragma unroll
  for (int r = 0; r < 8; ++r) w[r * 8 + j] = v[r];                 // this thread's own column: nobody else reads it before the barrier
  __syncthreads();

  // the coefficients of the real blocks: 128 contiguous bytes a block, 16 a thread
  const int gby = (sub420 && comp == 0 ? ty * 2 : ty) + by, gbx = (sub420 && comp ? tx * 4 : tx * 8) + bx;
  const int rows_c = comp ? a.cb_rows : a.yb_rows, cols_c = comp ? a.cb_cols : a.yb_cols;
  if (a.coef && gby < rows_c && gbx < cols_c) {
    const long ny = (long)a.yb_rows * a.yb_cols, nc = (long)a.cb_rows * a.cb_cols;
    const long first = b * (ny + 2 * nc) + (comp ? ny + (comp - 1) * nc : 0) + (long)gby * cols_c + gbx;
    *(uint4*)(a.coef + first * 64 + j * 8) = *(const uint4*)(scoef + blk * 64 + j * 8);
  }

#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = w[j * 8 + c];
  idct_1d<18>(v);
  {
    uint2 s;
    s.x = (unsigned)range_limit(v[0]) | ((unsigned)range_limit(v[1]) << 8) | ((unsigned)range_limit(v[2]) << 16) | ((unsigned)range_limit(v[3]) << 24);
    s.y = (unsigned)range_limit(v[4]) | ((unsigned)range_limit(v[5]) << 8) | ((unsigned)range_limit(v[6]) << 16) | ((unsigned)range_limit(v[7]) << 24);
    *(uint2*)(samp + blk * 64 + j * 8) = s;                        // the samples of this row were consumed before the first barrier
  }

  __syncthreads();

  // ---- the decoded planes: item i = 8 bytes, consecutive threads on consecutive bytes of one plane row
  {
    int pcomp, prow, pbx;                                          // plane, row and 8-byte column of this thread's item inside the tile
    if (sub420) {
      if (tid < 128) { pcomp = 0; prow = tid >> 3; pbx = tid & 7; }
      else { const int t = tid - 128; pcomp = 1 + (t >> 5); prow = (t >> 2) & 7; pbx = t & 3; }
    } else {
      pcomp = tid >> 6; prow = (tid >> 3) & 7; pbx = tid & 7;
    }
    const int sblk = sub420 ? (pcomp == 0 ? (prow >> 3) * 8 + pbx : 16 + (pcomp - 1) * 4 + pbx) : pcomp * 8 + pbx;
    const int pgby = (sub420 && pcomp == 0 ? ty * 2 : ty) + (prow >> 3), pgbx = (sub420 && pcomp ? tx * 4 : tx * 8) + pbx;
    if (pgby < (pcomp ? a.cb_rows : a.yb_rows) && pgbx < (pcomp ? a.cb_cols : a.yb_cols)) {
      const int pw = pcomp ? a.wc : a.wy;
      const long plane = pcomp == 0 ? 0 : (long)a.hy * a.wy + (long)(pcomp - 1) * a.hc * a.wc;
      const long gy = (long)(sub420 && pcomp ? ty * 8 : ty * a.th) + prow;
      *(uint2*)(a.planes + b * a.plane_stride + plane + gy * pw + (long)pgbx * 8) = *(const uint2*)(samp + sblk * 64 + (prow & 7) * 8);
    }
  }
}

// The chroma sample the decoder shows at pixel (y, x): libjpeg's h2v2 "fancy" upsampling over the plane cropped to ch x cw
DFH_DEVICE int fancy_chroma(const uint8_t* __restrict__ p, int pw, int ch, int cw, int y, int x) {
  const int cy = y >> 1, cx = x >> 1;
  const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const int fx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
  const uint8_t *near = p + (long)cy * pw, *far = p + (long)fy * pw;
  const int here = 3 * near[cx] + far[cx], next = 3 * near[fx] + far[fx];
  return (3 * here + next + ((x & 1) ? 7 : 8)) >> 4;
}

// The same for the four pixels 2 * cx0 .. 2 * cx0 + 3 of row y (w % 4 == 0, so chroma columns cx0 and cx0 + 1 are inside the cropped
// plane): the vertical blend of columns cx0 - 1 .. cx0 + 2 once, the middle two from one 16-bit read a row
DFH_DEVICE void fancy_chroma4(const uint8_t* __restrict__ p, int pw, int ch, int cw, int y, int cx0, int (&out)[4]) {
  const int cy = y >> 1;
  const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const uint8_t *near = p + (long)cy * pw, *far = p + (long)fy * pw;
  const int xl = max(cx0 - 1, 0), xr = min(cx0 + 2, cw - 1);
  const int n = *(const uint16_t*)(near + cx0), f = *(const uint16_t*)(far + cx0);
  const int s0 = 3 * near[xl] + far[xl], s1 = 3 * (n & 255) + (f & 255), s2 = 3 * (n >> 8) + (f >> 8), s3 = 3 * near[xr] + far[xr];
  out[0] = (3 * s1 + s0 + 8) >> 4;
  out[1] = (3 * s1 + s2 + 7) >> 4;
  out[2] = (3 * s2 + s1 + 8) >> 4;
  out[3] = (3 * s2 + s3 + 7) >> 4;
}

// PX = 4: four pixels of one row a thread, three aligned 4-byte stores (w % 4 == 0);  PX = 1: any width, byte stores
template <int PX>
__global__ __launch_bounds__(PIXELS_THREADS) void jpeg_pixels_kernel(const JpegArgs a) {
  const long i = (long)blockIdx.x * PIXELS_THREADS + threadIdx.x;
  const int per_row = a.w / PX;
  const long rows = (long)a.batch * a.h;
  if (i >= rows * per_row) return;
  const long rowi = i / per_row;
  const int x0 = (int)(i - rowi * per_row) * PX;
  const long b = rowi / a.h;
  const int y = (int)(rowi - b * a.h);
  const uint8_t* py = a.planes + b * a.plane_stride;
  const uint8_t* pcb = py + (long)a.hy * a.wy;
  const uint8_t* pcr = pcb + (long)a.hc * a.wc;
  int yv4[PX], cb4[PX], cr4[PX];
  if constexpr (PX == 4) {
    // x0 is a multiple of 4 and the planes' rows are multiples of 32 bytes: Y (and 4:4:4 chroma) as one dword, the two chroma columns
    // these four pixels sit on as one 16-bit read a row
    const uint32_t y4 = *(const uint32_t*)(py + (long)y * a.wy + x0);
    uint32_t b4 = 0, r4 = 0;
    if (a.sub420) {
      fancy_chroma4(pcb, a.wc, a.ch, a.cw, y, x0 >> 1, cb4);
      fancy_chroma4(pcr, a.wc, a.ch, a.cw, y, x0 >> 1, cr4);
    } else {
      b4 = *(const uint32_t*)(pcb + (long)y * a.wc + x0);
      r4 = *(const uint32_t*)(pcr + (long)y * a.wc + x0);
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      yv4[k] = (int)((y4 >> (8 * k)) & 255u);
      if (!a.sub420) { cb4[k] = (int)((b4 >> (8 * k)) & 255u); cr4[k] = (int)((r4 >> (8 * k)) & 255u); }
    }
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int x = x0 + k;
      yv4[k] = py[(long)y * a.wy + x];
      cb4[k] = a.sub420 ? fancy_chroma(pcb, a.wc, a.ch, a.cw, y, x) : pcb[(long)y * a.wc + x];
      cr4[k] = a.sub420 ? fancy_chroma(pcr, a.wc, a.ch, a.cw, y, x) : pcr[(long)y * a.wc + x];
    }
  }
  unsigned out[PX * 3];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int yv = yv4[k], cb = cb4[k] - 128, cr = cr4[k] - 128;
    const int r = yv + ((91881 * cr + 32768) >> 16);
    const int g = yv + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    const int bl = yv + ((116130 * cb + 32768) >> 16);
    out[k * 3] = (unsigned)min(max(r, 0), 255); out[k * 3 + 1] = (unsigned)min(max(g, 0), 255); out[k * 3 + 2] = (unsigned)min(max(bl, 0), 255);
  }
  uint8_t* o = a.dst + (rowi * a.w + x0) * 3;
  if (PX == 4) {
    uint32_t* o4 = (uint32_t*)o;
#pragma unroll
    for (int k = 0; k < 3; ++k) o4[k] = out[4 * k] | (out[4 * k + 1] << 8) | (out[4 * k + 2] << 16) | (out[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (uint8_t)out[k];
  }
}

// ---- host
const int LUMA_BASE[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                           14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const int CHROMA_BASE[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                             47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// libjpeg's jpeg_quality_scaling + jpeg_add_quant_table with force_baseline
int scaled_q(int base, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int q = (base * s + 50) / 100;
  return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// The geometry of one call: filled the same way for the size query and the launch
bool geometry(int batch, int h, int w, int subsampling, JpegArgs& a) {
  if (batch < 1 || h < 1 || w < 1 || h > 65536 || w > 65536) return false;
  if (subsampling != DFH_JPEG_SUBSAMPLING_420 && subsampling != DFH_JPEG_SUBSAMPLING_444) return false;
  a.batch = batch; a.h = h; a.w = w;
  a.sub420 = subsampling == DFH_JPEG_SUBSAMPLING_420;
  a.th = a.sub420 ? 16 : 8;
  a.tiles_x = (w + TILE_W - 1) / TILE_W; a.tiles_y = (h + a.th - 1) / a.th;
  a.ch = a.sub420 ? (h + 1) / 2 : h; a.cw = a.sub420 ? (w + 1) / 2 : w;
  a.yb_rows = (h + 7) / 8; a.yb_cols = (w + 7) / 8; a.cb_rows = (a.ch + 7) / 8; a.cb_cols = (a.cw + 7) / 8;
  a.wy = a.tiles_x * TILE_W; a.hy = a.tiles_y * a.th;
  a.wc = a.sub420 ? a.wy / 2 : a.wy; a.hc = a.sub420 ? a.hy / 2 : a.hy;
  a.plane_stride = (long)a.hy * a.wy + 2L * a.hc * a.wc;
  return true;
}

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

using dfh::aligned16;

}  // namespace

extern "C" {

int dfh_jpeg_quant_tables(int quality, int* luma64, int* chroma64) {
  DFH_REQUIRE(luma64 && chroma64, "null argument");
  DFH_REQUIRE(quality >= 1 && quality <= 100, "quality must be in [1, 100], got " + std::to_string(quality));
  for (int i = 0; i < 64; ++i) {
    luma64[i] = scaled_q(LUMA_BASE[i], quality);
    chroma64[i] = scaled_q(CHROMA_BASE[i], quality);
  }
  return 0;
}

size_t dfh_jpeg_workspace_bytes(int batch, int h, int w, int subsampling) {
  JpegArgs a;
  if (!geometry(batch, h, w, subsampling, a)) {
    dfh::set_error("dfh_jpeg_workspace_bytes: batch, h, w must be positive (h, w at most 65536) and subsampling 4:2:0 (2) or 4:4:4 (0)");
    return 0;
  }
  return (size_t)batch * (size_t)a.plane_stride;
}

size_t dfh_jpeg_coef_count(int batch, int h, int w, int subsampling) {
  JpegArgs a;
  if (!geometry(batch, h, w, subsampling, a)) {
    dfh::set_error("dfh_jpeg_coef_count: batch, h, w must be positive (h, w at most 65536) and subsampling 4:2:0 (2) or 4:4:4 (0)");
    return 0;
  }
  return (size_t)batch * 64 * ((size_t)a.yb_rows * a.yb_cols + 2 * (size_t)a.cb_rows * a.cb_cols);
}

int dfh_jpeg_roundtrip(const void* src, int src_kind, int batch, int h, int w, int quality, int subsampling, uint8_t* dst_hwc, int16_t* coef,
                       void* workspace, size_t workspace_bytes, void* stream) {
  DFH_REQUIRE(quality >= 1 && quality <= 100, "quality must be in [1, 100], got " + std::to_string(quality));
  DFH_REQUIRE(subsampling == DFH_JPEG_SUBSAMPLING_420 || subsampling == DFH_JPEG_SUBSAMPLING_444,
              "subsampling must be 4:2:0 (2) or 4:4:4 (0) in PIL's numbering, got " + std::to_string(subsampling) +
              ": 4:2:2 and the other layouts are not built");
  DFH_REQUIRE(batch >= 1 && h >= 1 && w >= 1, "batch, h and w must be positive");
  DFH_REQUIRE(h <= 65536 && w <= 65536, "h and w may be at most 65536 (JPEG's own limit is 65535)");
  DFH_REQUIRE(src_kind == DFH_IMGPROC_SRC_U8_HWC || src_kind == DFH_IMGPROC_SRC_F32_CHW, "src_kind must be 0 (uint8 HWC) or 1 (fp32 CHW)");
  DFH_REQUIRE(src && dst_hwc && workspace, "null argument (src / dst_hwc / workspace; coef alone may be null)");
  DFH_REQUIRE(aligned16(src) && aligned16(dst_hwc) && aligned16(coef) && aligned16(workspace), "src / dst_hwc / coef / workspace must be 16-byte aligned");
  JpegArgs a;
  DFH_REQUIRE(geometry(batch, h, w, subsampling, a), "internal: geometry");
  const size_t need = dfh_jpeg_workspace_bytes(batch, h, w, subsampling);
  DFH_REQUIRE(workspace_bytes >= need, "workspace smaller than dfh_jpeg_workspace_bytes (" + std::to_string(workspace_bytes) + " < " +
              std::to_string(need) + ")");
  const size_t px = (size_t)batch * h * w * 3, src_bytes = px * (src_kind == DFH_IMGPROC_SRC_U8_HWC ? 1 : 4);
  const size_t coef_bytes = coef ? dfh_jpeg_coef_count(batch, h, w, subsampling) * sizeof(int16_t) : 0;
  DFH_REQUIRE(!overlap(src, src_bytes, dst_hwc, px), "dst_hwc overlaps src: the round trip is not in place");
  DFH_REQUIRE(!overlap(workspace, need, src, src_bytes) && !overlap(workspace, need, dst_hwc, px), "workspace overlaps src or dst_hwc");
  DFH_REQUIRE(!coef || (!overlap(coef, coef_bytes, src, src_bytes) && !overlap(coef, coef_bytes, dst_hwc, px) &&
                        !overlap(coef, coef_bytes, workspace, need)), "coef overlaps src, dst_hwc or workspace");
  const long tiles = (long)batch * a.tiles_y * a.tiles_x;
  const int px_per_thread = w % 4 == 0 ? 4 : 1;
  const long pixel_blocks = ((long)batch * h * (w / px_per_thread) + PIXELS_THREADS - 1) / PIXELS_THREADS;
  DFH_REQUIRE(tiles < (1L << 31) && pixel_blocks < (1L << 31), "batch too large for one launch");
  a.src = src; a.src_kind = src_kind; a.planes = (uint8_t*)workspace; a.coef = coef; a.dst = dst_hwc;
  int ql[64], qc[64];
  if (dfh_jpeg_quant_tables(quality, ql, qc) != 0) return -1;
  for (int i = 0; i < 64; ++i) { a.q[0][i] = (uint16_t)ql[i]; a.q[1][i] = (uint16_t)qc[i]; }
  hipStream_t s = (hipStream_t)stream;
  {
    dfh::ProfScope ps(dfh::PC_OTHER, 0.0, (double)src_bytes + (double)need + (double)coef_bytes, s);
    hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, s, a);
    if (dfh::check_launch("jpeg_blocks_kernel") != 0) return -1;
  }
  dfh::ProfScope ps(dfh::PC_OTHER, 0.0, (double)need + (double)px, s);
  if (px_per_thread == 4) hipLaunchKernelGGL(jpeg_pixels_kernel<4>, dim3((unsigned)pixel_blocks), dim3(PIXELS_THREADS), 0, s, a);
  else hipLaunchKernelGGL(jpeg_pixels_kernel<1>, dim3((unsigned)pixel_blocks), dim3(PIXELS_THREADS), 0, s, a);
  return dfh::check_launch("jpeg_pixels_kernel");
}

}  // extern "C"
