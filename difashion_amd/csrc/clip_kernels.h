// The fp32 building blocks of the CLIP text tower (clip.hip) that the vision tower (clip_vision.hip) runs too: one definition of the
// kernels (in clip.hip), two callers.
#pragma once
#include "dfh_common.h"

namespace dfh {
enum { CLIP_ACT_NONE = 0, CLIP_ACT_QUICK_GELU = 1, CLIP_ACT_GELU = 2 };

// out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) (+ resid[m][n]) on v_mfma_f32_16x16x4_f32; W is nn.Linear layout [N][K] read in
// place (K a multiple of 4, rows 16-byte aligned), bias / resid may be null, resid may alias out.  prof_class: the dfh::ProfClass the
// launch is timed under.
int clip_linear(const float* A, int lda, const float* W, int K, const float* bias, const float* resid, int ld_res, float* out,
                int ld_out, int M, int N, int act, int prof_class, hipStream_t s);
// y[m][:] = LayerNorm(x[m * ldx : m * ldx + D]) * g + b, dense output rows; D a multiple of 4, x and y distinct buffers
int clip_layernorm(const float* x, long ldx, const float* g, const float* b, float* y, int M, int D, float eps, hipStream_t s);
}  // namespace dfh
