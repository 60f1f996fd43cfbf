// CLIP image preprocessing: what open_clip's / transformers' transform does to an image in front of the tower --
// PIL's antialiased 8-bit resize, a centre crop, ToTensor + Normalize -- in ONE launch.
//
// Replaces (arithmetic):
//   * PIL.Image.resize for 8-bit images as Pillow's Resample.c computes it: per axis a table of 22-bit integer coefficients made in
//     double on the host (dfh_imgproc::axis_tables below), a horizontal pass, then a vertical pass, each clip8((2^21 + sum pixel * k) >> 22)
//     in 32-bit integers, with the image between the passes held as CLIPPED uint8;
//   * transformers' centre crop, top = (h - crop_h) / 2, left = (w - crop_w) / 2;
//   * (v / 255 - mean) / std as a 3 x 256 fp32 table the caller hands in, so the kernel is integer arithmetic plus one table read.
//
// One workgroup owns (image, band of output rows).  It stages the source rows that band's vertical taps reach into LDS with aligned
// 16-byte loads, runs the horizontal pass over them for the columns the crop keeps into an LDS image of clipped bytes, runs the vertical
// pass out of that image, looks the result up and stores planar fp32 with consecutive lanes on consecutive x of one channel.  The
// image between the passes never reaches HBM.  Integers and fp32 only, the same in both storage builds; no atomics.
//
// This file is compiled with -ffp-contract=off (Makefile): the coefficient tables follow Pillow's expression order in double, and the
// fp32 source form's quantisation follows torch's separate ops.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "../../include/difashion_hip.h"
#include "dfh_common.h"

namespace {

constexpr int PRECISION_BITS = 22;
constexpr int THREADS = 256;
constexpr int LDS_BUDGET = 64 * 1024;         // bytes a workgroup may take: the row image between the passes + the staged source rows
constexpr int STAGE_TARGET = 16 * 1024;       // staged source rows a step, as far as they fit here
constexpr int MAX_BAND = 16, MAX_STAGE_ROWS = 8;

struct ImgArgs {
  const void* src; int src_kind; long src_bytes;
  int in_h, in_w, grid_n, g;                   // one item; items a sheet (>= 1); cells a sheet side
  int sh, sw;                                  // the (virtual) source image: g * in_h, g * in_w
  int out_h, out_w, top, left;
  int ksx, ksy;
  const int *bx, *cx, *by, *cy;                // bounds [n][2], coefficients [n][ksize] of the two axes
  const float* lut; float* pv; uint8_t* u8;
  int band, nbands, max_rows, row_stride, stage_rows, slot;
};

DFH_DEVICE int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
DFH_DEVICE int clip8(int acc) { return clampi(acc >> PRECISION_BITS, 0, 255); }

// The item that row r of cell gx of the sheet of output image b comes from, and its row yi in it; < 0: a white cell
DFH_DEVICE long cell_item(const ImgArgs& a, int b, int r, int gx, int& yi) {
  const int gy = a.g == 1 ? 0 : r / a.in_h;
  yi = r - gy * a.in_h;
  const int cell = gy * a.g + gx;
  if (cell >= a.grid_n) return -1;
  return (long)b * a.grid_n + cell;
}
// where the staged bytes of (sheet row r, cell gx) begin inside their slot: the uint8 form keeps the source's offset inside its
// 16-byte line, so that aligned global loads land on aligned LDS stores
DFH_DEVICE int cell_row_shift(const ImgArgs& a, int b, int r, int gx) {
  if (a.src_kind != DFH_IMGPROC_SRC_U8_HWC) return 0;
  int yi;
  const long item = cell_item(a, b, r, gx, yi);
  if (item < 0) return 0;
  return (int)((((item * a.in_h + yi) * a.in_w) * 3) & 15);
}

// difashion.postprocess(x, "pil"): x / 2 + 0.5, clamp to [0, 1], * 255, round half to even; NaN -> 0
DFH_DEVICE uint8_t quantise(float x) {
  float y = x * 0.5f + 0.5f;
  y = (y != y) ? 0.0f : fminf(fmaxf(y, 0.0f), 1.0f);
  return (uint8_t)(int)rintf(y * 255.0f);
}

// The one fetch: sheet rows r0 .. r0 + ns - 1 of output image b -> stage, one slot of interleaved RGB bytes per (row, cell)
DFH_DEVICE void fetch_rows(const ImgArgs& a, int b, int r0, int ns, uint8_t* stage, int tid) {
  if (a.src_kind == DFH_IMGPROC_SRC_U8_HWC) {
    const int nch = a.slot >> 4, len = a.in_w * 3;
    const uint8_t* base = (const uint8_t*)a.src;
    for (int i = tid; i < ns * a.g * nch; i += THREADS) {
      const int seg = i / nch, k = i - seg * nch;
      const int rr = seg / a.g, gx = seg - rr * a.g;
      int yi;
      const long item = cell_item(a, b, r0 + rr, gx, yi);
      uint4* dst = (uint4*)(stage + (long)seg * a.slot + k * 16);
      if (item < 0) { *dst = make_uint4(~0u, ~0u, ~0u, ~0u); continue; }      // white
      const long A = ((item * a.in_h + yi) * a.in_w) * 3;
      const long c0 = (A & ~15L) + k * 16;                                     // this thread's 16 bytes of the tensor
      if (c0 >= A + len) continue;                                             // behind the row
      if (c0 + 16 <= a.src_bytes) {
        *dst = *(const uint4*)(base + c0);
      } else {                                                                 // the tensor ends inside the line
        uint8_t* d8 = (uint8_t*)dst;
        for (int j = 0; j < 16; ++j) d8[j] = c0 + j < a.src_bytes ? base[c0 + j] : 0;
      }
    }
  } else {
    const float* base = (const float*)a.src;
    for (int rc = 0; rc < ns * 3; ++rc) {
      const int rr = rc / 3, c = rc - rr * 3;
      for (int x = tid; x < a.sw; x += THREADS) {
        const int gx = a.g == 1 ? 0 : x / a.in_w, xi = x - gx * a.in_w;
        int yi;
        const long item = cell_item(a, b, r0 + rr, gx, yi);
        const uint8_t v = item < 0 ? (uint8_t)255 : quantise(base[((item * 3 + c) * a.in_h + yi) * a.in_w + xi]);
        stage[(long)(rr * a.g + gx) * a.slot + xi * 3 + c] = v;
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void imgproc_kernel(const ImgArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint8_t* inter = smem;                                         // [max_rows][row_stride]: horizontally resized rows, clipped bytes
  uint8_t* stage = smem + (long)a.max_rows * a.row_stride;       // [stage_rows][g][slot]
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.nbands, band = blockIdx.x - b * a.nbands;
  const int oy0 = band * a.band, oy1 = min(oy0 + a.band, a.out_h);
  // the source rows this band's vertical taps reach; every index that comes out of a table is clamped before it addresses anything
  const int r_first = clampi(a.by[2 * (a.top + oy0)], 0, a.sh - 1);
  const int last = a.top + oy1 - 1;
  const int r_end = clampi(a.by[2 * last] + a.by[2 * last + 1], r_first + 1, a.sh);
  const int nrows = min(r_end - r_first, a.max_rows);

  for (int r0 = r_first; r0 < r_first + nrows; r0 += a.stage_rows) {
    const int ns = min(a.stage_rows, r_first + nrows - r0);
    __syncthreads();                                             // the previous step's readers of stage are done
    fetch_rows(a, b, r0, ns, stage, tid);
    __syncthreads();
    for (int i = tid; i < ns * a.out_w; i += THREADS) {
      const int rr = i / a.out_w, x = i - rr * a.out_w, ox = a.left + x;
      const int xmin = clampi(a.bx[2 * ox], 0, a.sw - 1);
      const int cnt = clampi(a.bx[2 * ox + 1], 0, min(a.ksx, a.sw - xmin));
      const int* k = a.cx + (long)ox * a.ksx;
      int gx = a.g == 1 ? 0 : xmin / a.in_w, xi = xmin - gx * a.in_w;
      const uint8_t* row = stage + (long)rr * a.g * a.slot;
      const uint8_t* p = row + gx * a.slot + cell_row_shift(a, b, r0 + rr, gx) + xi * 3;
      int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
      if (a.g == 1) {
        // a plain image: every thread runs all ksx taps, so the loop unrolls and its loads overlap -- the table holds zeros behind a
        // row's last tap (fill_tables), and such a tap re-reads the last pixel
        const int lastp = max(cnt - 1, 0) * 3;
#pragma unroll 4
        for (int t = 0; t < a.ksx; ++t) {
          const int kv = k[t], o = min(t * 3, lastp);
          s0 += __mul24((int)p[o], kv); s1 += __mul24((int)p[o + 1], kv); s2 += __mul24((int)p[o + 2], kv);
        }
      } else {
        for (int t = 0; t < cnt; ++t) {
          const int kv = k[t];
          s0 += __mul24((int)p[0], kv); s1 += __mul24((int)p[1], kv); s2 += __mul24((int)p[2], kv);
          p += 3;
          if (++xi == a.in_w && gx + 1 < a.g) {                  // the taps cross into the next cell of the sheet
            xi = 0; ++gx;
            p = row + gx * a.slot + cell_row_shift(a, b, r0 + rr, gx);
          }
        }
      }
      uint8_t* o = inter + (long)(r0 - r_first + rr) * a.row_stride + x * 3;
      o[0] = (uint8_t)clip8(s0); o[1] = (uint8_t)clip8(s1); o[2] = (uint8_t)clip8(s2);
    }
  }
  __syncthreads();

  const int per_row = 3 * a.out_w;
  for (int i = tid; i < (oy1 - oy0) * per_row; i += THREADS) {
    const int ol = i / per_row, rem = i - ol * per_row, c = rem / a.out_w, x = rem - c * a.out_w;
    const int oy = oy0 + ol, ry = a.top + oy;
    const int ymin = clampi(a.by[2 * ry], r_first, r_first + nrows - 1);
    const int cnt = clampi(a.by[2 * ry + 1], 0, min(a.ksy, r_first + nrows - ymin));
    const int* k = a.cy + (long)ry * a.ksy;
    const uint8_t* p = inter + (long)(ymin - r_first) * a.row_stride + x * 3 + c;
    int s = 1 << (PRECISION_BITS - 1);
    const int lastt = max(cnt - 1, 0);
#pragma unroll 4
    for (int t = 0; t < a.ksy; ++t) s += __mul24((int)p[min(t, lastt) * a.row_stride], k[t]);      // zeros behind the last tap, as above
    const int v = clip8(s);
    if (a.pv) a.pv[(((long)b * 3 + c) * a.out_h + oy) * a.out_w + x] = a.lut[c * 256 + v];
    if (a.u8) a.u8[(((long)b * a.out_h + oy) * a.out_w + x) * 3 + c] = (uint8_t)v;
  }
}

// ---- host: the plan
double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

struct AxisTables { int ksize = 0; std::vector<int> bounds, coef; };

}  // namespace

struct dfh_imgproc {
  dfh_imgproc_config cfg;
  int in_h, in_w, grid_n, g, sh, sw, rh, rw, out_h, out_w, top, left;
  AxisTables x, y;
  int row_stride, slot, stage_rows, fit_rows;

  // Pillow's precompute_coeffs + normalize_coeffs_8bpc, in its order of operations
  static bool axis_tables(int in_size, int out_size, int resample, AxisTables& t) {
    double (*filter)(double) = resample == 3 ? bicubic_filter : bilinear_filter;
    const double fsupport = resample == 3 ? 2.0 : 1.0;
    double filterscale, scale;
    filterscale = scale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = fsupport * filterscale;
    t.ksize = (int)std::ceil(support) * 2 + 1;
    t.bounds.assign((size_t)out_size * 2, 0);
    t.coef.assign((size_t)out_size * t.ksize, 0);
    std::vector<double> k((size_t)t.ksize);
    for (int xx = 0; xx < out_size; ++xx) {
      const double center = (xx + 0.5) * scale;
      double ww = 0.0;
      const double ss = 1.0 / filterscale;
      int xmin = (int)(center - support + 0.5);
      if (xmin < 0) xmin = 0;
      int xmax = (int)(center + support + 0.5);
      if (xmax > in_size) xmax = in_size;
      xmax -= xmin;
      for (int x = 0; x < xmax; ++x) {
        const double w = filter((x + xmin - center + 0.5) * ss);
        k[x] = w;
        ww += w;
      }
      for (int x = 0; x < xmax; ++x)
        if (ww != 0.0) k[x] /= ww;
      t.bounds[2 * xx] = xmin;
      t.bounds[2 * xx + 1] = xmax;
      for (int x = 0; x < xmax; ++x) {
        const int kv = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << PRECISION_BITS));
        if (kv <= -(1 << 23) || kv >= (1 << 23)) return false;               // the 24-bit multiply of the kernel
        t.coef[(size_t)xx * t.ksize + x] = kv;
      }
    }
    return true;
  }

  // source rows the band of R output rows with the widest reach needs
  int rows_needed(int R) const {
    int worst = 0;
    for (int oy0 = 0; oy0 < out_h; oy0 += R) {
      const int lastr = top + std::min(oy0 + R, out_h) - 1;
      worst = std::max(worst, y.bounds[2 * lastr] + y.bounds[2 * lastr + 1] - y.bounds[2 * (top + oy0)]);
    }
    return worst;
  }
  int band_rows(int batch) const {
    int R = 1;
    for (int c = MAX_BAND; c >= 1; --c)
      if (rows_needed(c) <= fit_rows) { R = c; break; }
    // a small batch: more, lower bands -- as long as the lower band fits too (its bands are not nested in the higher one's, so on an
    // upscale one of them can reach a row more)
    while (R > 4 && (long)batch * ((out_h + R - 1) / R) < 512 && rows_needed((R + 1) / 2) <= fit_rows) R = (R + 1) / 2;
    return R;
  }
  size_t table_ints() const { return x.bounds.size() + x.coef.size() + y.bounds.size() + y.coef.size(); }
};

extern "C" {

int dfh_imgproc_create(const dfh_imgproc_config* cfg, int in_h, int in_w, int grid_n, dfh_imgproc** out) {
  DFH_REQUIRE(cfg && out, "null argument");
  DFH_REQUIRE(cfg->resample == 3 || cfg->resample == 2, "unsupported resample filter " + std::to_string(cfg->resample) +
              ": PIL numbering, 3 (bicubic) or 2 (bilinear)");
  DFH_REQUIRE(in_h >= 1 && in_w >= 1 && in_h <= 16384 && in_w <= 16384, "in_h / in_w must be in [1, 16384]");
  DFH_REQUIRE(grid_n >= 0 && grid_n <= 64, "grid_n must be in [0, 64]");
  DFH_REQUIRE(cfg->shortest_edge >= 1 && cfg->shortest_edge <= 4096, "shortest_edge must be in [1, 4096]");
  DFH_REQUIRE((cfg->crop_height == 0) == (cfg->crop_width == 0) && cfg->crop_height >= 0 && cfg->crop_width >= 0,
              "crop_height / crop_width must both be positive, or both 0 (no crop)");
  dfh_imgproc* p = new (std::nothrow) dfh_imgproc();
  DFH_REQUIRE(p != nullptr, "out of host memory");
  p->cfg = *cfg; p->in_h = in_h; p->in_w = in_w; p->grid_n = grid_n > 0 ? grid_n : 1;
  int g = 1;
  while (g * g < p->grid_n) ++g;
  p->g = g; p->sh = g * in_h; p->sw = g * in_w;
  // transformers' get_resize_output_image_size: the short edge to shortest_edge, the other to int(shortest_edge * long / short)
  const int shortv = std::min(p->sh, p->sw), longv = std::max(p->sh, p->sw);
  const int new_long = (int)((double)((long)cfg->shortest_edge * longv) / (double)shortv);
  if (p->sw <= p->sh) { p->rw = cfg->shortest_edge; p->rh = new_long; } else { p->rh = cfg->shortest_edge; p->rw = new_long; }
  auto refuse = [&](const std::string& msg) { delete p; dfh::set_error("dfh_imgproc_create: " + msg); return -1; };
  if (p->rh > 16384 || p->rw > 16384) return refuse("the resized image exceeds 16384 pixels a side");
  p->out_h = cfg->crop_height ? cfg->crop_height : p->rh;
  p->out_w = cfg->crop_width ? cfg->crop_width : p->rw;
  if (p->rh < p->out_h || p->rw < p->out_w)
    return refuse("the resized image (" + std::to_string(p->rh) + " x " + std::to_string(p->rw) + ") is smaller than the crop (" +
                  std::to_string(p->out_h) + " x " + std::to_string(p->out_w) + ")");
  p->top = (p->rh - p->out_h) / 2; p->left = (p->rw - p->out_w) / 2;
  if (!dfh_imgproc::axis_tables(p->sw, p->rw, cfg->resample, p->x) || !dfh_imgproc::axis_tables(p->sh, p->rh, cfg->resample, p->y))
    return refuse("a coefficient does not fit 24 signed bits");
  // LDS: the rows between the passes (out_w * 3 bytes each) + the staged source rows (one 16-byte-aligned slot a cell)
  p->row_stride = (p->out_w * 3 + 15) & ~15;
  p->slot = (in_w * 3 + 15 + 15) & ~15;
  const long stage_row = (long)g * p->slot;
  p->stage_rows = (int)std::max(1L, std::min((long)MAX_STAGE_ROWS, STAGE_TARGET / stage_row));
  const long left_over = LDS_BUDGET - p->stage_rows * stage_row;
  p->fit_rows = left_over > 0 ? (int)(left_over / p->row_stride) : 0;
  if (p->rows_needed(1) > p->fit_rows)
    return refuse("this scale does not fit the kernel's LDS budget: one output row reaches " + std::to_string(p->rows_needed(1)) +
                  " source rows of " + std::to_string(p->row_stride) + " bytes next to " + std::to_string(stage_row) +
                  " bytes of staged source, 65536 in all (a 224-wide bicubic crop fits up to a scale of about 18)");
  *out = p;
  return 0;
}

void dfh_imgproc_destroy(dfh_imgproc* p) { delete p; }
int dfh_imgproc_resized_height(const dfh_imgproc* p) { return p ? p->rh : 0; }
int dfh_imgproc_resized_width(const dfh_imgproc* p) { return p ? p->rw : 0; }
int dfh_imgproc_out_height(const dfh_imgproc* p) { return p ? p->out_h : 0; }
int dfh_imgproc_out_width(const dfh_imgproc* p) { return p ? p->out_w : 0; }
int dfh_imgproc_crop_top(const dfh_imgproc* p) { return p ? p->top : 0; }
int dfh_imgproc_crop_left(const dfh_imgproc* p) { return p ? p->left : 0; }
int dfh_imgproc_ksize_x(const dfh_imgproc* p) { return p ? p->x.ksize : 0; }
int dfh_imgproc_ksize_y(const dfh_imgproc* p) { return p ? p->y.ksize : 0; }
size_t dfh_imgproc_table_bytes(const dfh_imgproc* p) { return p ? (p->table_ints() * sizeof(int) + 15) & ~(size_t)15 : 0; }

int dfh_imgproc_fill_tables(const dfh_imgproc* p, void* host_buffer, size_t buffer_bytes) {
  DFH_REQUIRE(p && host_buffer, "null argument");
  DFH_REQUIRE(buffer_bytes >= dfh_imgproc_table_bytes(p), "buffer smaller than dfh_imgproc_table_bytes");
  std::memset(host_buffer, 0, dfh_imgproc_table_bytes(p));
  int* o = (int*)host_buffer;
  for (const std::vector<int>* v : {&p->x.bounds, &p->x.coef, &p->y.bounds, &p->y.coef}) {
    std::memcpy(o, v->data(), v->size() * sizeof(int));
    o += v->size();
  }
  return 0;
}

int dfh_imgproc_run(const dfh_imgproc* p, const void* tables_dev, const float* lut_dev, const void* src, int src_kind, int batch,
                    float* pixel_values, uint8_t* out_u8, void* stream) {
  DFH_REQUIRE(p && tables_dev && src, "null argument");
  DFH_REQUIRE(pixel_values || out_u8, "null argument: pixel_values and out_u8 are both null");
  DFH_REQUIRE(!pixel_values || lut_dev, "null argument: pixel_values without the lookup table");
  DFH_REQUIRE(src_kind == DFH_IMGPROC_SRC_U8_HWC || src_kind == DFH_IMGPROC_SRC_F32_CHW, "src_kind must be 0 (uint8 HWC) or 1 (fp32 CHW)");
  DFH_REQUIRE(batch >= 1, "batch must be positive");
  DFH_REQUIRE((((uintptr_t)tables_dev | (uintptr_t)lut_dev | (uintptr_t)src | (uintptr_t)pixel_values) & 15) == 0,
              "tables / lut / src / pixel_values must be 16-byte aligned");
  ImgArgs a;
  a.band = p->band_rows(batch);
  a.nbands = (p->out_h + a.band - 1) / a.band;
  DFH_REQUIRE((long)batch * a.nbands < (1L << 31), "batch too large for one launch");
  a.src = src; a.src_kind = src_kind;
  a.src_bytes = (long)batch * p->grid_n * p->in_h * p->in_w * 3 * (src_kind == DFH_IMGPROC_SRC_U8_HWC ? 1 : 4);
  a.in_h = p->in_h; a.in_w = p->in_w; a.grid_n = p->grid_n; a.g = p->g; a.sh = p->sh; a.sw = p->sw;
  a.out_h = p->out_h; a.out_w = p->out_w; a.top = p->top; a.left = p->left; a.ksx = p->x.ksize; a.ksy = p->y.ksize;
  a.bx = (const int*)tables_dev; a.cx = a.bx + p->x.bounds.size(); a.by = a.cx + p->x.coef.size(); a.cy = a.by + p->y.bounds.size();
  a.lut = lut_dev; a.pv = pixel_values; a.u8 = out_u8;
  a.max_rows = p->rows_needed(a.band); a.row_stride = p->row_stride; a.stage_rows = p->stage_rows; a.slot = p->slot;
  const size_t lds = (size_t)a.max_rows * a.row_stride + (size_t)a.stage_rows * p->g * p->slot;
  DFH_REQUIRE(lds <= (size_t)LDS_BUDGET, "internal: the band does not fit the LDS budget");
  hipStream_t s = (hipStream_t)stream;
  const double out_px = (double)batch * p->out_h * p->out_w * 3;
  dfh::ProfScope ps(dfh::PC_OTHER, 0.0, (double)a.src_bytes + out_px * ((pixel_values ? 4 : 0) + (out_u8 ? 1 : 0)), s);
  hipLaunchKernelGGL(imgproc_kernel, dim3((unsigned)(batch * a.nbands)), dim3(THREADS), lds, s, a);
  dfh::census(dfh::CK_IMGPROC);
  return dfh::check_launch("imgproc_kernel");
}

}  // extern "C"
