// The device-resident item store: the VAE posterior of every item, computed once, kept in HBM as one fp32 row
// [mean | std] per item; the model's inputs are then two row gathers a step instead of 33 encoder passes and 32 host copies.
//
// Replaces (arithmetic) what DiFashion.forward / fashion_generation do with `vae.encode(images).latent_dist` (difashion.py:123-136,
// :180-184) and the per-row dict lookups of pre-averaged history latents (data_utils.py:142-155):
//
//   item_gather_kernel    out[r] = (mean[iid_r] + std[iid_r] * eps[r]) * scale   -- latent_dist.sample() * sf;  eps absent: mode() * sf
//   history_rows_kernel   out[r] = (sum_k table[item_k] * scale, in list order) / count   -- the mean of a user's history items of one
//                         category, from the SAME table: no materialised per-segment mean table (tens of GB on the real data sets)
//
// Every result is a chain of separate IEEE fp32 operations (this file is compiled with -ffp-contract=off, as elementwise.hip is), so
// the store path reproduces the torch expressions of the image path bit for bit.  fp32 only: the fp16-storage library gives the same
// bits.  No atomics, nothing allocated, no scratch, no workspace, one launch each.
//
// Layout: a lane owns ONE float4 of the output row and consecutive lanes own consecutive 16 B, so every table row is read as whole
// 1 KiB-per-wave lines; the grid is (row, 256-lane slab of the row).  Row offsets are 64-bit: iid * row_stride passes 2^31 elements at
// 65 537 moment rows of 4 x 64 x 64.
#include <cmath>

#include "../../include/difashion_hip.h"
#include "dfh_common.h"

namespace {

constexpr int SLAB_LANES = 256;        // one workgroup = 256 float4 = 4 KiB of a row
constexpr int HIST_UNROLL = 4;         // item loads in flight per lane

DFH_DEVICE float4 nan4() {
  const float n = __uint_as_float(0x7fc00000u);
  return make_float4(n, n, n, n);
}

__global__ __launch_bounds__(SLAB_LANES) void item_gather_kernel(const float* __restrict__ table, long table_rows, long row_stride, int row_elems,
                                                                 const int64_t* __restrict__ iids, const float* __restrict__ eps, float scale,
                                                                 float* __restrict__ out) {
  const int c = blockIdx.y * SLAB_LANES + threadIdx.x;       // this lane's float4 of the row
  if (c * 4 >= row_elems) return;
  const long r = blockIdx.x;
  const int64_t iid = iids[r];
  float4* o = (float4*)(out + r * row_elems) + c;
  if (iid < 0 || iid >= table_rows) { *o = nan4(); return; }  // a bad id is visible and reads nothing
  const float* row = table + iid * row_stride;
  float4 v = ((const float4*)row)[c];
  if (eps) {
    const float4 s = ((const float4*)(row + row_elems))[c];
    const float4 e = ((const float4*)(eps + r * row_elems))[c];
    v.x = v.x + s.x * e.x; v.y = v.y + s.y * e.y; v.z = v.z + s.z * e.z; v.w = v.w + s.w * e.w;
  }
  v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
  *o = v;
}

// the addend of one history item: the item's float4 of means (an id outside the table adds NaN and reads nothing)
DFH_DEVICE float4 hist_load(const float* __restrict__ table, long table_rows, long row_stride, int64_t iid, int c) {
  if (iid < 0 || iid >= table_rows) return nan4();
  return ((const float4*)(table + iid * row_stride))[c];
}

DFH_DEVICE void hist_add(float4& acc, const float4 v, float scale) {
  acc.x = acc.x + v.x * scale; acc.y = acc.y + v.y * scale; acc.z = acc.z + v.z * scale; acc.w = acc.w + v.w * scale;
}

__global__ __launch_bounds__(SLAB_LANES) void history_rows_kernel(const float* __restrict__ table, long table_rows, long row_stride, int row_elems,
                                                                  const int64_t* __restrict__ seg_items, const int64_t* __restrict__ seg_offsets,
                                                                  const int* __restrict__ row_seg, const float* __restrict__ null_row, float scale,
                                                                  float* __restrict__ out) {
  const int c = blockIdx.y * SLAB_LANES + threadIdx.x;
  if (c * 4 >= row_elems) return;
  const long r = blockIdx.x;
  float4* o = (float4*)(out + r * row_elems) + c;
  const int seg = row_seg[r];
  int64_t first = 0, count = 0;
  if (seg >= 0) { first = seg_offsets[seg]; count = seg_offsets[seg + 1] - first; }
  if (count <= 0) { *o = ((const float4*)null_row)[c]; return; }
  const int64_t* items = seg_items + first;      // wave-uniform: the ids arrive through the scalar cache
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int64_t k = 0;
  for (; k + HIST_UNROLL <= count; k += HIST_UNROLL) {
    float4 v[HIST_UNROLL];
#pragma unroll
    for (int u = 0; u < HIST_UNROLL; ++u) v[u] = hist_load(table, table_rows, row_stride, items[k + u], c);   // four loads in flight ...
#pragma unroll
    for (int u = 0; u < HIST_UNROLL; ++u) hist_add(acc, v[u], scale);                                         // ... added in list order
  }
  for (; k < count; ++k) hist_add(acc, hist_load(table, table_rows, row_stride, items[k], c), scale);
  const float n = (float)count;
  acc.x = acc.x / n; acc.y = acc.y / n; acc.z = acc.z / n; acc.w = acc.w / n;
  *o = acc;
}

using dfh::aligned16;

}  // namespace

extern "C" {

int dfh_item_gather(const float* table, long table_rows, long row_stride, int row_elems, const int64_t* iids, long rows, const float* eps,
                    float scale, float* out, void* stream) {
  DFH_REQUIRE(table && iids && out, "null argument (table / iids / out; eps alone may be null: the mode)");
  DFH_REQUIRE(table_rows >= 0 && rows >= 0 && row_elems > 0, "negative table_rows / rows, or row_elems not positive");
  DFH_REQUIRE(row_elems % 4 == 0 && row_stride % 4 == 0, "row_elems and row_stride must be multiples of 4 (rows are read as float4)");
  DFH_REQUIRE(row_stride >= row_elems, "row_stride smaller than row_elems");
  DFH_REQUIRE(!eps || row_stride >= 2L * row_elems, "row_stride smaller than 2 * row_elems: a means-only table has no std half for eps");
  DFH_REQUIRE(aligned16(table) && aligned16(out) && aligned16(eps), "table / eps / out must be 16-byte aligned");
  DFH_REQUIRE(rows <= 0x7fffffffL && row_elems <= 65535 * SLAB_LANES * 4, "rows beyond 2^31 - 1 or row_elems beyond 65535 slabs of 1024");
  if (rows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  dfh::ProfScope ps(dfh::PC_OTHER, 0.0, 4.0 * (double)rows * row_elems * (eps ? 4 : 2), s);
  const int slabs = (row_elems / 4 + SLAB_LANES - 1) / SLAB_LANES;
  hipLaunchKernelGGL(item_gather_kernel, dim3((unsigned)rows, slabs), dim3(SLAB_LANES), 0, s, table, table_rows, row_stride, row_elems, iids, eps,
                     scale, out);
  return dfh::check_launch("item_gather_kernel");
}

int dfh_history_rows(const float* table, long table_rows, long row_stride, int row_elems, const int64_t* seg_items, const int64_t* seg_offsets,
                     const int* row_seg, long rows, const float* null_row, float scale, float* out, void* stream) {
  DFH_REQUIRE(table && seg_items && seg_offsets && row_seg && null_row && out, "null argument");
  DFH_REQUIRE(table_rows >= 0 && rows >= 0 && row_elems > 0, "negative table_rows / rows, or row_elems not positive");
  DFH_REQUIRE(row_elems % 4 == 0 && row_stride % 4 == 0, "row_elems and row_stride must be multiples of 4 (rows are read as float4)");
  DFH_REQUIRE(row_stride >= row_elems, "row_stride smaller than row_elems");
  DFH_REQUIRE(aligned16(table) && aligned16(out) && aligned16(null_row), "table / null_row / out must be 16-byte aligned");
  DFH_REQUIRE(rows <= 0x7fffffffL && row_elems <= 65535 * SLAB_LANES * 4, "rows beyond 2^31 - 1 or row_elems beyond 65535 slabs of 1024");
  if (rows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  dfh::ProfScope ps(dfh::PC_OTHER, 0.0, 0.0, s);           // the bytes depend on the segments, which live on the device
  const int slabs = (row_elems / 4 + SLAB_LANES - 1) / SLAB_LANES;
  hipLaunchKernelGGL(history_rows_kernel, dim3((unsigned)rows, slabs), dim3(SLAB_LANES), 0, s, table, table_rows, row_stride, row_elems, seg_items,
                     seg_offsets, row_seg, null_row, scale, out);
  return dfh::check_launch("history_rows_kernel");
}

}  // extern "C"
